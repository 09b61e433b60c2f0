"""featurize of UTF-8 in byte space through the batch flow (latok_flow_token_features_utf8_bytes), modelled on
test_gpu_flow_utf8.py: a batch is enqueued without any wait and must come out bit-identical to the blocking call
(latok_token_features_utf8_bytes_batch, which test_gpu_features_utf8_bytes.py pins to the oracle) -- counts, the 4-field byte
records, the 25 sums, and the four result words (token total, error word, code-point total, malformed flag)."""
import random

import numpy as np
import pytest

from conftest import ALPHABETS, RULE_SETS, pack, random_strings
from test_gpu_features_utf8 import _edge_text
from test_gpu_flow_utf8 import ALPHA, POISON, SCAN_BLOCK, TILE, _Arena, _Job, _batches, _resident

pytestmark = pytest.mark.gpu

DTYPES = (np.int64, np.int32)
SOFT = [b"ab\xe6\x97 cd", b"\xc3 x", b"lone \xf0\x9f\x98", b"end\xe6", b"next starts ascii", b"\xe6\x97\xa5\xe6", b"\xf0", b"x\xc3"]
HARD = [b"a\x80\x80\x80\x80b", b"\xa9 starts with a continuation byte"]


class _BJob(_Job):
    """one resident UTF-8 batch through the byte-space featurize form: poisoned counts / records / sums, four result words"""

    def __init__(self, ar, d_u8, d_boff, n_str, nbytes, dt=np.int64, cap=None):
        super().__init__(ar, d_u8, d_boff, n_str, nbytes, "features", dt, cap)

    def submit(self, total=None):
        from latok_amd import batch
        batch.flow_token_features_utf8_bytes(self.d_u8, self.d_boff, self.n_str, self.nbytes if total is None else total, self.d_counts,
                                             self.d_items, self.d_feat, self.cap, self.d_res, dtype=self.dt)

    def untouched(self):
        isz = np.dtype(self.dt).itemsize
        return bool((self.ar.get(self.d_items, self.cap * 4 * isz, np.uint8) == POISON).all() and
                    (self.ar.get(self.d_feat, self.cap * 25, np.uint8) == POISON).all())


def _blocking(u8, boff, dt):
    from latok_amd import batch
    return batch.token_features_utf8_bytes_csr(u8, boff, dtype=dt)


def _total_cps(u8):
    return int(((u8 & 0xC0) != 0x80).sum())


def _check(job, want, total_cps, what=""):
    res, counts, items, feats = job.records()
    w_counts, w_items, w_feats = want
    assert res[0] == len(w_items) and res[2] == total_cps, (what, res)
    assert np.array_equal(counts, w_counts) and np.array_equal(items, w_items) and np.array_equal(feats, w_feats), (what, job.dt)


def test_sixteen_batches_in_flight_equal_the_blocking_call(gpu):
    """sixteen batches from one byte to several segments, every one with buffers of its own (so they alternate between the two
    slots and overlap), int64 and int32 records, total_bytes given and -1"""
    from latok_amd import batch
    rng = random.Random(2026)
    ar = _Arena(gpu)
    try:
        work = []
        for texts in _batches(rng) + _batches(rng):
            u8, boff, d_u8, d_boff = _resident(ar, texts)
            work.append((texts, u8, boff, d_u8, d_boff, {dt: _blocking(u8, boff, dt) for dt in DTYPES}))
        sizes = [w[1].size for w in work]
        assert len(work) == 16 and min(sizes) == 1 and sum(s <= 262144 for s in sizes) >= 8 and max(sizes) > 2 * 262144
        for dt, total in ((np.int64, None), (np.int32, -1), (np.int32, None)):
            jobs = [_BJob(ar, d_u8, d_boff, len(texts), u8.size, dt) for texts, u8, _, d_u8, d_boff, _ in work]
            for j in jobs:
                j.submit(total)
            batch.flow_wait()
            for k, (j, w) in enumerate(zip(jobs, work)):
                _check(j, w[5][dt], _total_cps(w[1]), (k, dt, total))
    finally:
        ar.free()


def test_consecutive_batches_that_reuse_the_same_output_buffers(gpu):
    """the ordering rule: three different batches write the same counts / records / sums / result words back to back, with an
    unrelated batch in between; after one wait the buffers hold the LAST one's results, and the unrelated batch its own"""
    from latok_amd import batch
    rng = random.Random(8)
    ta, tb, tc, tx = (random_strings(rng, n, 0, m, ALPHA) for n, m in ((12000, 300), (900, 120), (5000, 200), (700, 90)))
    ar = _Arena(gpu)
    try:
        (ua, oa, d_ua, d_oa), (ub, ob, d_ub, d_ob), (uc, oc, d_uc, d_oc), (ux, ox, d_ux, d_ox) = (_resident(ar, t) for t in (ta, tb, tc, tx))
        for dt in DTYPES:
            for last_u8, last_off, order in ((uc, oc, "abc"), (ub, ob, "acb")):
                shared = _BJob(ar, d_ua, d_oa, len(ta), ua.size, dt)      # the largest batch sizes the shared buffers
                other = _BJob(ar, d_ux, d_ox, len(tx), ux.size, dt)
                jobs = {"a": shared, "b": _BJob(ar, d_ub, d_ob, len(tb), ub.size, dt), "c": _BJob(ar, d_uc, d_oc, len(tc), uc.size, dt)}
                for k in "bc":
                    j = jobs[k]
                    j.d_counts, j.d_items, j.d_feat, j.d_res, j.cap = shared.d_counts, shared.d_items, shared.d_feat, shared.d_res, shared.cap
                jobs[order[0]].submit()
                other.submit()
                jobs[order[1]].submit()
                jobs[order[2]].submit()
                batch.flow_wait()
                _check(jobs[order[2]], _blocking(last_u8, last_off, dt), _total_cps(last_u8), ("reused", order, dt))
                _check(other, _blocking(ux, ox, dt), _total_cps(ux), ("unrelated", order, dt))
    finally:
        ar.free()


def test_capacity_protocol_read_late(gpu):
    from latok_amd import batch
    rng = random.Random(100)
    texts = random_strings(rng, 2500, 0, 150, ALPHA)
    ar = _Arena(gpu)
    try:
        u8, boff, d_u8, d_boff = _resident(ar, texts)
        want = _blocking(u8, boff, np.int32)
        need = len(want[1])
        short = _BJob(ar, d_u8, d_boff, len(texts), u8.size, np.int32, cap=need - 1)
        short.submit()
        batch.flow_wait()
        res = short.check_ok()
        assert res[0] == need > short.cap and res[2] == _total_cps(u8)                # too small: the needed count is reported,
        assert np.array_equal(ar.get(short.d_counts, len(texts), np.int32), want[0])   # counts are valid
        assert short.untouched()                                                      # and no record, no sum was written
        again = _BJob(ar, d_u8, d_boff, len(texts), u8.size, np.int32, cap=int(res[0]))
        again.submit()
        batch.flow_wait()
        _check(again, want, _total_cps(u8), "resubmitted")
    finally:
        ar.free()


def test_malformed_input_is_reported_and_the_next_batch_is_unaffected(gpu):
    """`soft` blobs: result[3] == 0 and the blocking call's results.  With the `hard` ones: result[3] != 0, record and sum
    buffers untouched -- and the next batch on the SAME slot (it shares the counts buffer, so it is ordered behind) is what the
    blocking call gives; the blocking call itself refuses the malformed bytes."""
    from latok_amd import batch
    rng = random.Random(0xBAD7)
    body = [t.encode("utf-8") for t in random_strings(rng, 3000, 0, 120, ALPHA)]
    good_texts = random_strings(rng, 2000, 0, 100, ALPHA)
    ar = _Arena(gpu)
    try:
        ug, og, d_ug, d_og = _resident(ar, good_texts)
        for extra, bad in ((SOFT, False), (SOFT + HARD, True), (HARD[:1], True), (HARD[1:], True)):
            blobs = body[:1500] + extra + body[1500:] + extra if len(extra) > 1 else ["well formed é".encode()] + extra + [b"tail"]
            u8, boff = batch.pack_utf8(blobs)
            d_u8, d_boff = ar.put(u8), ar.put(boff)
            for dt in DTYPES:
                job = _BJob(ar, d_u8, d_boff, len(blobs), u8.size, dt)
                nxt = _BJob(ar, d_ug, d_og, len(good_texts), ug.size, dt)
                job.d_counts = nxt.d_counts = ar.alloc(max(len(blobs), len(good_texts)) * 8, POISON)
                job.submit()
                nxt.submit()
                batch.flow_wait()
                if not bad:
                    want = _blocking(u8, boff, dt)
                    res = job.check_ok()
                    n = int(res[0])
                    assert n == len(want[1]) and res[2] == _total_cps(u8), (dt, res)
                    assert np.array_equal(ar.get(job.d_items, (n, 4), dt), want[1]) and np.array_equal(ar.get(job.d_feat, (n, 25), np.int8), want[2])
                    own = _BJob(ar, d_u8, d_boff, len(blobs), u8.size, dt)     # (the shared counts now hold the next batch's)
                    own.submit()
                    batch.flow_wait()
                    _check(own, want, _total_cps(u8), ("soft", dt))
                else:
                    res = job.res()
                    assert res[3] != 0 and job.untouched(), (dt, res)
                    with pytest.raises(ValueError, match="malformed UTF-8"):
                        _blocking(u8, boff, dt)
                _check(nxt, _blocking(ug, og, dt), _total_cps(ug), ("next batch on the slot", bad, dt))
    finally:
        ar.free()


def test_empty_batches_clear_result_words_and_counts(gpu):
    from latok_amd import batch
    ar = _Arena(gpu)
    try:
        d_u8, d_boff = ar.alloc(16), ar.put(np.zeros(6, np.int64))
        for total in (0, -1):
            job = _BJob(ar, d_u8, d_boff, 5, 0, np.int32)
            job.submit(total)
            batch.flow_wait()
            assert not job.res().any() and not ar.get(job.d_counts, 5, np.int32).any()
            assert (job.raw_items(4) == 0x7F7F7F7F).all()
        none = _BJob(ar, d_u8, d_boff, 0, 0)
        none.submit()
        batch.flow_wait()
        assert not none.res().any()
    finally:
        ar.free()


def test_edges_and_exact_totals(gpu):
    """the word / tile / workgroup edge text, the two dense-prefix batches, and batches whose code-point total is exactly one tile
    (from ASCII alone, and with multi-byte chars: the grids behind the lead scan are sized by the bytes and over-sized)"""
    from latok_amd import batch
    rng = random.Random(0xA5E)
    text = _edge_text()
    cuts = [0, 1000, 70001, 140003, 300007, len(text)]
    cases = [[text], [text[a:b] for a, b in zip(cuts[:-1], cuts[1:])]]
    for e in (640, 641):
        r2 = random.Random(e + 9)
        chars = ["é"] * e + [r2.choice("abc d.@") for _ in range(65536 - 2 * e)]
        r2.shuffle(chars)
        prefix = "".join(chars)
        tail = ("lorem ipsum #x a@b.c " * 10000)[:3 * 65536 + 37]
        cases += [[prefix + tail], [prefix[:100], prefix[100:] + tail[:5000], tail[5000:]]]
    body = "".join(rng.choice("ab c.é日🤓@") for _ in range(TILE))
    cases += [["ab c." * 819 + "x"], [body], [body[:1000], "", body[1000:]], [body + "y"], [body[:-1]]]
    cases.append(random_strings(rng, 3000, 0, 200, ALPHABETS["words"] + list("ABC,.:/!19\t")))
    ar = _Arena(gpu)
    try:
        work = []
        for texts in cases:
            u8, boff, d_u8, d_boff = _resident(ar, texts)
            work.append((u8, boff, [_BJob(ar, d_u8, d_boff, len(texts), u8.size, dt) for dt in DTYPES]))
        for _, _, jobs in work:
            for j in jobs:
                j.submit()
        batch.flow_wait()
        for k, (u8, boff, jobs) in enumerate(work):
            for j in jobs:
                _check(j, _blocking(u8, boff, j.dt), _total_cps(u8), ("edges", k))
    finally:
        ar.free()


@pytest.mark.parametrize("ascii_only", [True, False])
def test_a_code_point_total_of_exactly_one_scan_block(gpu, ascii_only):
    """4096 x 4096 code points = one full workgroup of the chained scan (an exact multiple of the 4096-tile block).  ASCII: all
    three scans cover exactly one block; with multi-byte chars the byte-space scans have a second workgroup and the code-point
    scan (sized by bytes) a surplus one behind the real total."""
    from latok_amd import batch
    rng = random.Random(12)
    period = random_strings(rng, 700, 0, 180, ALPHABETS["words"] if ascii_only else ALPHA)
    n = sum(len(t) for t in period)
    while n > 65536:
        n -= len(period.pop())
    period.append("p" * (65536 - n))
    reps = SCAN_BLOCK // 65536
    texts = period * reps
    ar = _Arena(gpu)
    try:
        u8, boff, d_u8, d_boff = _resident(ar, texts)
        assert _total_cps(u8) == SCAN_BLOCK and (u8.size == SCAN_BLOCK) == ascii_only
        up, op = batch.pack_utf8([t.encode("utf-8") for t in period])
        want = _blocking(up, op, np.int32)        # strings are independent: the batch is whole repeats of the period
        job = _BJob(ar, d_u8, d_boff, len(texts), u8.size, np.int32, cap=reps * len(want[1]))
        job.submit()
        batch.flow_wait()
        _check(job, (np.tile(want[0], reps), np.tile(want[1], (reps, 1)), np.tile(want[2], (reps, 1))), SCAN_BLOCK, "scan block")
    finally:
        ar.free()


def test_long_tokens(gpu):
    rng = random.Random(4244)
    n = 1_000_000
    body = "".join(rng.choice("abcdefghXYZ019_") for _ in range(n))
    docs = ["short one", "see http://" + body[:n - 11], "", "é" * 5000 + "@" + "日" * 200000 + " end", "🤓" * 300000, "tail #tag"]
    ar = _Arena(gpu)
    try:
        from latok_amd import batch
        u8, boff, d_u8, d_boff = _resident(ar, docs)
        jobs = [_BJob(ar, d_u8, d_boff, len(docs), u8.size, dt) for dt in DTYPES]
        for j in jobs:
            j.submit()
        batch.flow_wait()
        for j in jobs:
            _check(j, _blocking(u8, boff, j.dt), _total_cps(u8), "long tokens")
    finally:
        ar.free()


@pytest.mark.parametrize("name", ["sym_everywhere", "all_columns"])
def test_run_time_rule_tables(gpu, name):
    from latok_amd import batch
    rng = random.Random(0x5E9)
    ar = _Arena(gpu)
    batch.set_rules(*RULE_SETS[name])
    try:
        for texts in (random_strings(rng, 8000, 0, 80, ALPHA), random_strings(rng, 300, 0, 80, ALPHA)):
            u8, boff, d_u8, d_boff = _resident(ar, texts)
            cps, row = pack(texts)
            jobs = [_BJob(ar, d_u8, d_boff, len(texts), u8.size, dt) for dt in DTYPES]
            for j in jobs:
                j.submit()
            batch.flow_wait()
            for j in jobs:
                _check(j, _blocking(u8, boff, j.dt), _total_cps(u8), name)
                assert np.array_equal(j.records()[3], batch.token_features_csr(cps, row, dtype=j.dt)[2])
    finally:
        batch.reset_rules()
        ar.free()


def test_interleaved_with_the_code_point_form_in_one_flow(gpu):
    """byte-space and code-point featurize of the same batches alternate on the slots: both use the slot's lead / packed-mask /
    rule-code buffers and its rank arrays"""
    from latok_amd import batch
    rng = random.Random(2719)
    ar = _Arena(gpu)
    try:
        work = []
        for k in range(5):
            texts = random_strings(rng, 400 + 900 * k, 0, 60 + 50 * k, ALPHA)
            u8, boff, d_u8, d_boff = _resident(ar, texts)
            work.append((u8, boff, _BJob(ar, d_u8, d_boff, len(texts), u8.size, np.int32),
                         _Job(ar, d_u8, d_boff, len(texts), u8.size, "features", np.int32)))
        for _ in range(2):
            for _, _, jb, jc in work:
                jb.submit()
                jc.submit()
            batch.flow_wait()
            for u8, boff, jb, jc in work:
                _check(jb, _blocking(u8, boff, np.int32), _total_cps(u8), "interleaved")
                res, counts, items, feats = jc.records()
                wc, wi, wf = batch.token_features_utf8_csr(u8, boff, dtype=np.int32)
                assert np.array_equal(counts, wc) and np.array_equal(items, wi) and np.array_equal(feats, wf)
    finally:
        ar.free()


def test_refused_arguments(gpu):
    from latok_amd import batch
    with pytest.raises(ValueError):
        batch.flow_token_features_utf8_bytes(0x1000, 0x2000, 3, 10, 0x3000, 0x4000, 0x6000, 10, None)     # NULL result words
    with pytest.raises(ValueError):
        batch.flow_token_features_utf8_bytes(0x1004, 0x2000, 3, 10, 0x3000, 0x4000, 0x6000, 10, 0x5000)   # misaligned bytes
    with pytest.raises(ValueError):
        batch.flow_token_features_utf8_bytes(0x1000, 0x2000, 3, 10, 0x3000, 0x4000, None, 10, 0x5000)     # NULL feature sums
    with pytest.raises(ValueError):
        batch.flow_token_features_utf8_bytes(0x1000, 0x2000, 3, 10, 0x3000, 0x4000, 0x6000, -1, 0x5000)   # negative capacity
