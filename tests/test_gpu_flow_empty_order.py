"""An all-empty batch of a flow zeroes caller memory (the counts, for join also out_off) with plain memsets on its slot's stream.
Those memsets must be ordered against a batch in flight that writes the same buffer: the flow routes by the ranges a batch notes
(flow_hazards.h), and every submitter notes them before it enqueues anything (api.cpp: flow_open).  Here, for each of the four
submitters that zero caller memory -- flow_token_spans, flow_token_spans_utf8, flow_join_tokens_utf8_bytes,
flow_token_hashes_utf8_bytes -- a batch A of several tiles (its tile kernel is still running when the next call arrives) and an
all-empty batch B name the same counts buffer X, back to back, in both orders: A then B must leave X all zero, B then A must leave
A's counts in X; B's result words are zero and A's other outputs are what the blocking call gives.

Such a test can only catch a misordering, not prove its absence: two streams that nothing orders may still happen to run in the
order the test expects."""
import random

import numpy as np
import pytest

from conftest import ALPHABETS, pack, random_strings
from test_gpu_flow_utf8 import POISON, _Arena

pytestmark = pytest.mark.gpu

N_STR = 64
FORMS = ("spans", "spans_utf8", "join", "hashes")
RESULT_WORDS = {"spans": 2, "spans_utf8": 4, "join": 2, "hashes": 2}


@pytest.fixture(scope="module")
def batch_a(gpu):
    """batch A (64 strings, ~20 KB of mixed ASCII and multi-byte text: five tiles) and what the blocking calls give for it"""
    from latok_amd import batch
    rng = random.Random(20261017)
    texts = random_strings(rng, N_STR, 200, 300, ALPHABETS["mixed"] + list("éü日Ж") + ["http://a.b/c", "me@x.org", "#tag"])
    cps, row = pack(texts)
    u8, boff = batch.pack_utf8([t.encode("utf-8") for t in texts])
    assert cps.size > 2 * 4096 and u8.size > 2 * 4096
    want = {"spans": batch.token_spans_csr(cps, row), "spans_utf8": batch.token_spans_utf8_csr(u8, boff),
            "join": batch.join_tokens_utf8_csr(u8, boff), "hashes": batch.token_hashes_utf8_csr(u8, boff, spans=True)}
    return {"cps": cps, "row": row, "u8": u8, "boff": boff, "want": want}


class _Pair:
    """the device buffers of A and B: they share X (counts; for join also out_off), everything else is A's or B's own"""

    def __init__(self, ar, form, a):
        self.ar, self.form = ar, form
        utf8 = form != "spans"
        self.units, self.rows = (a["u8"], a["boff"]) if utf8 else (a["cps"], a["row"])
        self.total = int(self.rows[-1])
        self.d_units, self.d_rows = ar.put(self.units), ar.put(self.rows)
        self.d_rows_empty = ar.put(np.zeros(N_STR + 1, np.int64))
        self.d_counts = ar.alloc(N_STR * 8, POISON)                      # X
        self.d_out_off = ar.alloc((N_STR + 1) * 8, POISON)               # X of join
        self.cap = 2 * self.total if form == "join" else self.total
        self.d_items = ar.alloc(self.cap * 16, POISON)                   # spans [n, 2] int64, or the joined bytes
        self.d_hashes = ar.alloc(self.cap * 4, POISON)
        self.d_res = {"A": ar.alloc(32, POISON), "B": ar.alloc(32, POISON)}

    def submit(self, which):
        from latok_amd import batch
        rows, total, res = (self.d_rows, self.total, self.d_res["A"]) if which == "A" else (self.d_rows_empty, 0, self.d_res["B"])
        if self.form == "spans":
            batch.flow_token_spans(self.d_units, 4, rows, N_STR, total, self.d_counts, self.d_items, self.cap, res)
        elif self.form == "spans_utf8":
            batch.flow_token_spans_utf8(self.d_units, rows, N_STR, total, self.d_counts, self.d_items, self.cap, res)
        elif self.form == "join":
            batch.flow_join_tokens_utf8_bytes(self.d_units, rows, N_STR, total, self.d_items, self.cap, self.d_out_off, self.d_counts, res)
        else:
            batch.flow_token_hashes_utf8_bytes(self.d_units, rows, N_STR, total, self.d_counts, self.d_items, self.d_hashes, self.cap, res)

    def check(self, want, a_last):
        """after flow_wait: X, B's result words, A's result words and A's other outputs"""
        ar, form = self.ar, self.form
        counts = ar.get(self.d_counts, N_STR, np.int64)
        res_a = ar.get(self.d_res["A"], RESULT_WORDS[form], np.int64)
        assert not ar.get(self.d_res["B"], RESULT_WORDS[form], np.int64).any()
        if form == "join":
            w_out, w_off, w_counts = want
            out_off = ar.get(self.d_out_off, N_STR + 1, np.int64)
            assert res_a.tolist() == [w_out.size, 0]
            assert np.array_equal(ar.get(self.d_items, w_out.size, np.uint8), w_out)
            assert np.array_equal(out_off, w_off) if a_last else not out_off.any()
        else:
            w_counts, w_hashes, w_spans = want if form == "hashes" else (want[0], None, want[1])
            n = int(w_counts.sum())
            assert res_a[:2].tolist() == [n, 0]
            if form == "spans_utf8":
                assert res_a[2:].tolist() == [int(_total_cps(self.units)), 0]
            assert np.array_equal(ar.get(self.d_items, (n, 2), np.int64), w_spans)
            if form == "hashes":
                assert np.array_equal(ar.get(self.d_hashes, n, np.uint32), w_hashes)
        assert w_counts.any()
        assert np.array_equal(counts, w_counts) if a_last else not counts.any()


def _total_cps(u8):
    """code points of a well-formed UTF-8 buffer: its bytes that are no continuation bytes"""
    return np.count_nonzero((u8 & 0xC0) != 0x80)


@pytest.mark.parametrize("order", ("A_then_B", "B_then_A"))
@pytest.mark.parametrize("form", FORMS)
def test_empty_batch_is_ordered_against_a_batch_in_flight(gpu, batch_a, form, order):
    from latok_amd import batch
    ar = _Arena(gpu)
    try:
        pair = _Pair(ar, form, batch_a)
        batch.flow_wait()
        for which in order.split("_then_"):
            pair.submit(which)
        batch.flow_wait()
        pair.check(batch_a["want"][form], a_last=order == "B_then_A")
    finally:
        batch.flow_wait()
        ar.free()
