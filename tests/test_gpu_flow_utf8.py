"""UTF-8 in code-point units through the batch flow (include/latok_hip.h: latok_flow_split_mask_utf8, _split_offsets_utf8,
_token_spans_utf8, _token_features_utf8).  A batch is enqueued without any wait: the stages behind the lead-byte scan read the
code-point total from device memory, and the malformed-input flag comes back in result[3].  Every result must be what the oracle
gives for the decoded text (mask, offsets, spans, parse-matrix sums) and what the blocking _utf8_batch calls give for the same
bytes.  Every well-formed case asserts result[3] == 0 and result[1] == 0 (``_Job.check_ok``): nothing passes by a fallback."""
import random
import threading

import numpy as np
import pytest

from conftest import ALPHABETS, RULE_SETS, pack, random_strings
from helpers import utf8_ref
from test_gpu_features_utf8 import _edge_text, _oracle_raw

pytestmark = pytest.mark.gpu

TILE, SCAN_BLOCK = 4096, 4096 * 4096      # chars per tile; chars per workgroup of the chained scan (4096 tile counts)
DTYPES = (np.int64, np.int32)
EXTRA = list("é日🤓ü　Жδ𝒳漢") + ["http://a.b/c?d=1", "see me@x.org", "#tag", ".@you", "a@b.c"]
ALPHA = ALPHABETS["mixed"] + EXTRA
WIDTH = {"offsets": 1, "spans": 2, "features": 4}
POISON = 0x7F


def _enc(texts):
    from latok_amd import batch
    return batch.pack_utf8([t.encode("utf-8", "surrogatepass") for t in texts])


class _Arena:
    """device allocations of one test"""

    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def alloc(self, nbytes, poison=None):
        from latok_amd import _lib
        size = max(int(nbytes), 16) + 64
        p = self.lib.latok_dev_alloc(size)
        assert p
        self.ptrs.append(p)
        if poison is not None:
            # latok_memset_dev is enqueued on the context's own stream, which nothing orders against the flow's streams: wait for
            # it here (a small blocking read on that stream; it leaves batches in flight alone), or it could land after a result
            _lib.check(self.lib.latok_memset_dev(p, poison, size))
            _lib.check(self.lib.latok_memcpy_d2h(np.empty(1, np.int64).ctypes.data, p, 8))
        return p

    def put(self, a):
        from latok_amd import _lib
        p = self.alloc(a.nbytes)
        if a.nbytes:
            _lib.check(self.lib.latok_memcpy_h2d(p, a.ctypes.data, a.nbytes))
        return p

    def get(self, p, shape, dt):
        from latok_amd import _lib
        out = np.empty(shape, dt)
        if out.nbytes:
            _lib.check(self.lib.latok_memcpy_d2h(out.ctypes.data, p, out.nbytes))
        return out

    def free(self):
        for p in self.ptrs:
            self.lib.latok_dev_free(p)
        self.ptrs = []


class _Job:
    """one form of one resident UTF-8 batch: its (poisoned) outputs and four result words"""

    def __init__(self, ar, d_u8, d_boff, n_str, nbytes, form, dt=np.int64, cap=None):
        self.ar, self.d_u8, self.d_boff, self.n_str, self.nbytes, self.form, self.dt = ar, d_u8, d_boff, n_str, nbytes, form, dt
        isz = np.dtype(dt).itemsize
        self.d_res = ar.alloc(32, POISON)
        if form == "mask":
            self.cap = (nbytes + 63) // 64 if cap is None else cap
            self.d_mask = ar.alloc(self.cap * 8, POISON)
            self.d_row = ar.alloc((n_str + 1) * 8, POISON)
        else:
            self.cap = nbytes if cap is None else cap
            self.d_counts = ar.alloc(n_str * isz, POISON)
            self.d_items = ar.alloc(self.cap * WIDTH[form] * isz, POISON)
            self.d_feat = ar.alloc(self.cap * 25, POISON) if form == "features" else None

    def submit(self, total=None):
        from latok_amd import batch
        total = self.nbytes if total is None else total
        if self.form == "mask":
            batch.flow_split_mask_utf8(self.d_u8, self.d_boff, self.n_str, total, self.d_mask, self.cap, self.d_row, self.d_res)
        elif self.form == "offsets":
            batch.flow_split_offsets_utf8(self.d_u8, self.d_boff, self.n_str, total, self.d_counts, self.d_items, self.cap, self.d_res, dtype=self.dt)
        elif self.form == "spans":
            batch.flow_token_spans_utf8(self.d_u8, self.d_boff, self.n_str, total, self.d_counts, self.d_items, self.cap, self.d_res, dtype=self.dt)
        else:
            batch.flow_token_features_utf8(self.d_u8, self.d_boff, self.n_str, total, self.d_counts, self.d_items, self.d_feat, self.cap,
                                           self.d_res, dtype=self.dt)

    def res(self):
        return self.ar.get(self.d_res, 4, np.int64)

    def check_ok(self):
        """a well-formed batch: not reported as malformed, no scan error, no int32 overflow"""
        res = self.res()
        assert res[3] == 0 and res[1] == 0, (self.form, res)
        return res

    def mask(self):
        res = self.check_ok()
        return res, self.ar.get(self.d_mask, (int(res[2]) + 63) // 64, np.uint64), self.ar.get(self.d_row, self.n_str + 1, np.int64)

    def records(self):
        res = self.check_ok()
        n, w = int(res[0]), WIDTH[self.form]
        assert n <= self.cap
        items = self.ar.get(self.d_items, (n, w) if w > 1 else n, self.dt)
        feats = self.ar.get(self.d_feat, (n, 25), np.int8) if self.form == "features" else None
        return res, self.ar.get(self.d_counts, self.n_str, self.dt), items, feats

    def raw_items(self, n_values):
        return self.ar.get(self.d_items, n_values, self.dt)


def _expect(oracle, texts, feats=True):
    """what the oracle gives for the decoded text: mask words and row offsets, offsets, stripped token spans and (feats) the raw
    spans + the parse-matrix sums of the kept tokens"""
    cps, row = pack(texts)
    vals, bits = oracle.split_batch(cps, row)
    o_counts, offs, t_counts, spans = [], [], [], []
    for i, t in enumerate(texts):
        nz = np.nonzero(vals[row[i]:row[i + 1]])[0]
        assert np.array_equal(nz, oracle.split_offsets(t)) if (t and i < 40) else True     # split_batch == the per-string oracle
        o_counts.append(len(nz))
        offs.append(nz)
        k = 0
        for a, b in zip(nz.tolist(), nz.tolist()[1:] + [len(t)]):
            tok = t[a:b]
            s = tok.strip()
            if s:
                lead = len(tok) - len(tok.lstrip())
                spans.append((a + lead, a + lead + len(s)))
                k += 1
        t_counts.append(k)
    e = {"cps": cps, "row": row, "bits": bits, "total": int(row[-1]), "o_counts": np.array(o_counts, np.int64),
         "offs": np.concatenate(offs).astype(np.int64) if offs else np.zeros(0, np.int64), "t_counts": np.array(t_counts, np.int64),
         "spans": np.array(spans, np.int64).reshape(-1, 2)}
    if feats:
        c, raw, f = _oracle_raw(oracle, texts)
        assert np.array_equal(c, e["t_counts"])
        e["raw"], e["feats"] = raw, f
    return e


def _check(job, e, what=""):
    """the job's results against the oracle's expectation `e`"""
    if job.form == "mask":
        res, bits, rowo = job.mask()
        assert res[0] == 0 and res[2] == e["total"], (what, res)
        assert np.array_equal(bits, e["bits"]) and np.array_equal(rowo, e["row"]), what
        return
    res, counts, items, feats = job.records()
    assert res[2] == e["total"], (what, res)
    if job.form == "offsets":
        assert res[0] == e["offs"].size and np.array_equal(counts, e["o_counts"]) and np.array_equal(items, e["offs"]), (what, job.dt)
    elif job.form == "spans":
        assert res[0] == len(e["spans"]) and np.array_equal(counts, e["t_counts"]) and np.array_equal(items, e["spans"]), (what, job.dt)
    else:
        assert res[0] == len(e["spans"]) and np.array_equal(counts, e["t_counts"]), (what, job.dt)
        assert np.array_equal(items[:, 2:], e["spans"]), (what, job.dt)
        if "raw" in e:
            assert np.array_equal(items[:, :2], e["raw"]) and np.array_equal(feats, e["feats"]), (what, job.dt)


def _check_blocking(job, u8, boff, what=""):
    """the job's results against the blocking _utf8_batch call on the same bytes"""
    from latok_amd import batch
    if job.form == "mask":
        res, bits, rowo = job.mask()
        wb, wr = batch.split_mask_utf8_csr(u8, boff)
        assert res[2] == wr[-1] and np.array_equal(bits, wb) and np.array_equal(rowo, wr), what
        return
    res, counts, items, feats = job.records()
    if job.form == "offsets":
        wc, wi = batch.split_offsets_utf8_csr(u8, boff, dtype=job.dt)
    elif job.form == "spans":
        wc, wi = batch.token_spans_utf8_csr(u8, boff, dtype=job.dt)
    else:
        wc, wi, wf = batch.token_features_utf8_csr(u8, boff, dtype=job.dt)
        assert np.array_equal(feats, wf), (what, job.dt)
    assert res[0] == len(wi) and np.array_equal(counts, wc) and np.array_equal(items, wi.reshape(items.shape)), (what, job.form, job.dt)


def _resident(ar, texts):
    u8, boff = _enc(texts)
    return u8, boff, ar.put(u8), ar.put(boff)


def _run_all_forms(gpu, oracle, texts, what, dts=DTYPES, feats=True, blocking=False, totals=(None,)):
    """the four forms of one batch, all in one flow, against the oracle (and the blocking calls)"""
    from latok_amd import batch
    ar = _Arena(gpu)
    try:
        u8, boff, d_u8, d_boff = _resident(ar, texts)
        e = _expect(oracle, texts, feats)
        for total in totals:
            jobs = [_Job(ar, d_u8, d_boff, len(texts), u8.size, "mask")]
            jobs += [_Job(ar, d_u8, d_boff, len(texts), u8.size, f, dt) for dt in dts for f in ("offsets", "spans", "features")]
            for j in jobs:
                j.submit(total)
            batch.flow_wait()
            for j in jobs:
                _check(j, e, what)
                if blocking:
                    _check_blocking(j, u8, boff, what)
        return e
    finally:
        ar.free()


def _batches(rng):
    """the shapes of test_gpu_flow.py::_batches over the mixed alphabet + astral and CJK extras: from a one-byte batch to several
    segments, most of them at or below 262 144 bytes"""
    out = [["x"], ["", "a b", ""], random_strings(rng, 50, 0, 40, ALPHA),
           random_strings(rng, 3000, 0, 200, ALPHA),
           random_strings(rng, 4, 30000, 90000, ALPHABETS["rare_space_at"] + ["日", "🤓"]) + random_strings(rng, 200, 0, 100, ALPHABETS["starts"] + ["é"]),
           random_strings(rng, 2, 200000, 400000, ALPHABETS["nospace_at"] + ["漢"]) + ["@a b"],
           random_strings(rng, 20000, 0, 60, ALPHABETS["words"] + ["é", "日本", "🤓"]),
           random_strings(rng, 700, 0, 64, ALPHA)]
    rng.shuffle(out)
    return out


def test_sixteen_batches_back_to_back_equal_the_oracle(gpu, oracle):
    """sixteen batches of very different sizes through one flow, every form of every batch, int64 and int32 records;
    total_bytes given, then -1"""
    from latok_amd import batch
    rng = random.Random(2025)
    ar = _Arena(gpu)
    try:
        work = []
        for texts in _batches(rng) + _batches(rng):
            u8, boff, d_u8, d_boff = _resident(ar, texts)
            work.append((texts, _expect(oracle, texts), u8, boff, d_u8, d_boff))
        sizes = [w[2].size for w in work]
        assert len(work) == 16 and min(sizes) == 1 and sum(s <= 262144 for s in sizes) >= 8 and max(sizes) > 2 * 262144
        for dt, total in ((np.int64, None), (np.int32, -1), (np.int32, None)):
            jobs = [[_Job(ar, d_u8, d_boff, len(texts), u8.size, f, dt) for f in ("mask", "offsets", "spans", "features")]
                    for texts, _, u8, _, d_u8, d_boff in work]
            for js in jobs:
                for j in js:
                    j.submit(total)
            batch.flow_wait()
            for k, (js, (_, e, u8, boff, _, _)) in enumerate(zip(jobs, work)):
                for j in js:
                    _check(j, e, (k, dt, total))
                    if u8.size > 262144 and total is None:
                        _check_blocking(j, u8, boff, k)
    finally:
        ar.free()


def test_edges_of_words_tiles_and_workgroups(gpu, oracle):
    text = _edge_text()
    cuts = [0, 1000, 70001, 140003, 300007, len(text)]
    for texts in ([text], [text[a:b] for a, b in zip(cuts[:-1], cuts[1:])]):
        _run_all_forms(gpu, oracle, texts, "edges", blocking=True)
    # a mixed prefix of exactly 16 tiles whose lead count is / is not a multiple of 64, then a dense-ASCII tail
    for e in (640, 641):
        a = 65536 - 2 * e
        rng = random.Random(e)
        chars = ["é"] * e + [rng.choice("abc d.@") for _ in range(a)]
        rng.shuffle(chars)
        prefix = "".join(chars)
        assert len(prefix.encode()) == 65536 and (len(prefix) % 64 == 0) == (e == 640)
        tail = ("lorem ipsum #x a@b.c " * 10000)[:3 * 65536 + 37]
        for texts in ([prefix + tail], [prefix[:100], prefix[100:] + tail[:5000], tail[5000:]]):
            _run_all_forms(gpu, oracle, texts, ("dense", e), dts=(np.int32,), blocking=True)


def test_all_ascii_empty_strings_and_exact_totals(gpu, oracle):
    from latok_amd import batch
    rng = random.Random(0xA5C)
    _run_all_forms(gpu, oracle, random_strings(rng, 3000, 0, 200, ALPHABETS["words"] + list("ABC,.:/!19\t")), "ASCII", dts=(np.int32,))
    # a code-point total of exactly one tile: from ASCII alone (bytes == chars) and with multi-byte chars (more bytes than chars)
    body = "".join(rng.choice("ab c.é日🤓@") for _ in range(TILE))
    for texts in (["ab c." * 819 + "x"], [body], [body[:1000], "", body[1000:]], [body + "y"], [body[:-1]]):
        e = _run_all_forms(gpu, oracle, texts, "one tile", dts=(np.int64,))
        assert abs(e["total"] - TILE) <= 1
    # only empty strings: nothing is launched, the result words, counts and row offsets are cleared on the slot's stream
    ar = _Arena(gpu)
    try:
        d_u8, d_boff = ar.alloc(16), ar.put(np.zeros(6, np.int64))
        jobs = [_Job(ar, d_u8, d_boff, 5, 0, f, np.int32) for f in ("mask", "offsets", "spans", "features")]
        for j in jobs:
            j.submit()
        jobs[1].submit(-1)
        batch.flow_wait()
        assert not jobs[0].res().any() and not ar.get(jobs[0].d_row, 6, np.int64).any()
        for j in jobs[1:]:
            assert not j.res().any() and not ar.get(j.d_counts, 5, np.int32).any()
            assert (j.raw_items(4) == 0x7F7F7F7F).all()
        none = _Job(ar, d_u8, d_boff, 0, 0, "offsets")
        none.submit()
        batch.flow_wait()
        assert not none.res().any()
    finally:
        ar.free()


def test_a_code_point_total_of_zero_is_reported_as_malformed(gpu):
    """bytes without a single lead byte: the only way to a code-point total of 0 with bytes present.  The downstream grids are
    sized by the byte count and find no work; the chained scan over 0 tiles still completes (result[1] == 0)."""
    from latok_amd import batch
    ar = _Arena(gpu)
    try:
        u8 = np.full(3 * TILE + 5, 0x80, np.uint8)
        boff = np.array([0, 100, 100, u8.size], np.int64)
        d_u8, d_boff = ar.put(u8), ar.put(boff)
        jobs = [_Job(ar, d_u8, d_boff, 3, u8.size, f, np.int64) for f in ("mask", "offsets", "spans", "features")]
        for j in jobs:
            j.submit()
        batch.flow_wait()
        for j in jobs:
            res = j.res()
            assert res[3] != 0 and res[2] == 0 and res[1] == 0 and res[0] == 0, (j.form, res)
        for j in jobs[1:]:
            assert (j.raw_items(16).view(np.uint8) == POISON).all()
    finally:
        ar.free()


@pytest.mark.parametrize("ascii_only", [True, False])
def test_a_code_point_total_of_exactly_one_scan_block(gpu, oracle, ascii_only):
    """4096 x 4096 code points = one full workgroup of the chained scan.  ASCII: the lead-byte scan and the item scan both cover
    exactly one block; with multi-byte chars the grids (sized by bytes) have a surplus workgroup behind the real total, which
    publishes an empty aggregate.  The batch is whole repeats of one oracle-checked period (strings are independent)."""
    from latok_amd import batch
    rng = random.Random(11)
    period = random_strings(rng, 700, 0, 180, ALPHABETS["words"] if ascii_only else ALPHA)
    n = sum(len(t) for t in period)
    period = [t for t in period]
    while n > 65536:
        n -= len(period.pop())
    period.append("p" * (65536 - n))
    e = _expect(oracle, period, feats=False)
    reps = SCAN_BLOCK // 65536
    texts = period * reps
    ar = _Arena(gpu)
    try:
        u8, boff, d_u8, d_boff = _resident(ar, texts)
        assert (u8.size == SCAN_BLOCK) == ascii_only
        jobs = [_Job(ar, d_u8, d_boff, len(texts), u8.size, f, np.int32) for f in ("mask", "offsets", "spans", "features")]
        for j in jobs:
            j.submit()
        batch.flow_wait()
        res, bits, rowo = jobs[0].mask()
        assert res[2] == SCAN_BLOCK and np.array_equal(bits, np.tile(e["bits"], reps))
        assert np.array_equal(rowo[1:].reshape(reps, -1) - (np.arange(reps) * 65536)[:, None], np.tile(e["row"][1:], (reps, 1)))
        res, counts, items, _ = jobs[1].records()
        assert res[0] == reps * e["offs"].size and np.array_equal(counts, np.tile(e["o_counts"], reps)) and np.array_equal(items, np.tile(e["offs"], reps))
        res, counts, items, _ = jobs[2].records()
        assert res[0] == reps * len(e["spans"]) and np.array_equal(counts, np.tile(e["t_counts"], reps)) and np.array_equal(items, np.tile(e["spans"], (reps, 1)))
        for j in jobs[1:]:
            _check_blocking(j, u8, boff, "scan block")
    finally:
        ar.free()


def test_long_tokens_under_featurize(gpu, oracle):
    """a 1 M-char token and a string of 300 000 astral chars"""
    rng = random.Random(4242)
    n = 1_000_000
    body = "".join(rng.choice("abcdefghXYZ019_") for _ in range(n))
    docs = ["short one", "see http://" + body[:n - 11], "", "é" * 5000 + "@" + "日" * 200000 + " end", "🤓" * 300000, "tail #tag"]
    _run_all_forms(gpu, oracle, docs, "long tokens", blocking=True)


@pytest.mark.parametrize("name", ["sym_everywhere", "all_columns"])
def test_run_time_rule_tables(gpu, oracle, name):
    """under latok_set_rules the flow's results are the blocking calls' (which the parity tests pin to the oracle under the same
    tables), and the mask is the oracle's for these tables"""
    from conftest import oracle_rule_bits
    from latok_amd import batch
    rng = random.Random(0x5E7)
    ar = _Arena(gpu)
    batch.set_rules(*RULE_SETS[name])
    try:
        for texts in (random_strings(rng, 8000, 0, 80, ALPHA), random_strings(rng, 300, 0, 80, ALPHA)):
            u8, boff, d_u8, d_boff = _resident(ar, texts)
            cps, row = pack(texts)
            jobs = [_Job(ar, d_u8, d_boff, len(texts), u8.size, "mask")]
            jobs += [_Job(ar, d_u8, d_boff, len(texts), u8.size, f, dt) for dt in DTYPES for f in ("offsets", "spans", "features")]
            for j in jobs:
                j.submit()
            batch.flow_wait()
            res, bits, rowo = jobs[0].mask()
            assert np.array_equal(bits, oracle_rule_bits(oracle, texts, RULE_SETS[name])) and np.array_equal(rowo, row)
            for j in jobs[1:]:
                res, counts, items, feats = j.records()
                if j.form == "offsets":
                    wc, wi = batch.split_offsets_csr(cps, row, dtype=j.dt)
                elif j.form == "spans":
                    wc, wi = batch.token_spans_csr(cps, row, dtype=j.dt)
                else:
                    wc, wi, wf = batch.token_features_csr(cps, row, dtype=j.dt)
                    assert np.array_equal(feats, wf)
                assert res[0] == len(wi) and np.array_equal(counts, wc) and np.array_equal(items, wi.reshape(items.shape)), (name, j.form)
    finally:
        batch.reset_rules()
        ar.free()


@pytest.mark.parametrize("form", ["offsets", "spans", "features"])
def test_capacity_protocol_read_late(gpu, oracle, form):
    from latok_amd import batch
    rng = random.Random(99)
    texts = random_strings(rng, 2500, 0, 150, ALPHA)
    e = _expect(oracle, texts)
    need = e["offs"].size if form == "offsets" else len(e["spans"])
    ar = _Arena(gpu)
    try:
        u8, boff, d_u8, d_boff = _resident(ar, texts)
        short = _Job(ar, d_u8, d_boff, len(texts), u8.size, form, np.int32, cap=need - 1)
        short.submit()
        batch.flow_wait()
        res = short.check_ok()
        assert res[0] == need > short.cap and res[2] == e["total"]                        # too small: the needed count is reported,
        assert np.array_equal(ar.get(short.d_counts, len(texts), np.int32), e["o_counts"] if form == "offsets" else e["t_counts"])   # counts are valid
        assert (short.raw_items(short.cap * WIDTH[form]) == 0x7F7F7F7F).all()                # and no record was written
        if form == "features":
            assert (ar.get(short.d_feat, short.cap * 25, np.uint8) == POISON).all()
        again = _Job(ar, d_u8, d_boff, len(texts), u8.size, form, np.int32, cap=int(res[0]))
        again.submit()
        batch.flow_wait()
        _check(again, e, "resubmitted")
    finally:
        ar.free()


def test_malformed_input_is_reported_not_decoded(gpu):
    """the blobs of test_gpu_features_utf8.py::test_malformed_input_equals_the_staged_decoder.  `soft`: cut-short sequences and
    lone leads that byte space and the staged decoder read alike -- result[3] == 0 and the staged decoder's results.  With the
    `hard` ones (continuation bytes without a lead within 3 bytes, a string that begins with one): result[3] != 0, the record
    buffers stay untouched, and the blocking call on the same bytes succeeds."""
    from latok_amd import batch
    rng = random.Random(0xBAD)
    body = [t.encode("utf-8") for t in random_strings(rng, 3000, 0, 120, ALPHA)]
    soft = [b"ab\xe6\x97 cd", b"\xc3 x", b"lone \xf0\x9f\x98", b"end\xe6", b"next starts ascii", b"\xe6\x97\xa5\xe6", b"\xf0", b"x\xc3"]
    hard = [b"a\x80\x80\x80\x80b", b"\xa9 starts with a continuation byte"]
    ar = _Arena(gpu)
    try:
        for extra, bad in ((soft, False), (soft + hard, True), (hard[:1], True), (hard[1:], True)):
            blobs = body[:1500] + extra + body[1500:] + extra if len(extra) > 1 else ["well formed é".encode()] + extra + [b"tail"]
            u8, boff = batch.pack_utf8(blobs)
            d_u8, d_boff = ar.put(u8), ar.put(boff)
            jobs = [_Job(ar, d_u8, d_boff, len(blobs), u8.size, "mask")]
            jobs += [_Job(ar, d_u8, d_boff, len(blobs), u8.size, f, dt) for dt in DTYPES for f in ("offsets", "spans", "features")]
            for j in jobs:
                j.submit()
            batch.flow_wait()
            cps, row = batch.utf8_decode_csr(u8, boff)                  # the staged decoder, held to the rule first
            want_cps, want_row, _ = utf8_ref.decode_batch(u8, boff)
            assert np.array_equal(cps, want_cps) and np.array_equal(row, want_row)
            if not bad:
                res, bits, rowo = jobs[0].mask()
                assert res[2] == row[-1] and np.array_equal(bits, batch.split_mask_batch(cps, row)) and np.array_equal(rowo, row)
                for j in jobs[1:]:
                    res, counts, items, feats = j.records()
                    if j.form == "offsets":
                        wc, wi = batch.split_offsets_csr(cps, row, dtype=j.dt)
                    elif j.form == "spans":
                        wc, wi = batch.token_spans_csr(cps, row, dtype=j.dt)
                    else:
                        wc, wi, wf = batch.token_features_csr(cps, row, dtype=j.dt)
                        assert np.array_equal(feats, wf)
                    assert res[0] == len(wi) and np.array_equal(counts, wc) and np.array_equal(items, wi.reshape(items.shape)), j.form
                    _check_blocking(j, u8, boff, "soft")
                continue
            for j in jobs:
                assert j.res()[3] != 0, j.form
            for j in jobs[1:]:
                assert (ar.get(j.d_items, j.cap * WIDTH[j.form] * np.dtype(j.dt).itemsize, np.uint8) == POISON).all(), j.form
                if j.form == "features":
                    assert (ar.get(j.d_feat, j.cap * 25, np.uint8) == POISON).all()
            # the caller's way out: the blocking call on the same bytes has the staged decoder
            wc, wi, wf = batch.token_features_utf8_csr(u8, boff, dtype=np.int32)
            c2, i2, f2 = batch.token_features_csr(cps, row, dtype=np.int32)
            assert np.array_equal(wc, c2) and np.array_equal(wi, i2) and np.array_equal(wf, f2)
    finally:
        ar.free()


def test_shared_outputs_end_with_the_last_batch(gpu, oracle):
    """two batches in flight that name the same records buffer, or only the same result words, are ordered: the shared memory
    ends with the LAST one's values, with an unrelated batch in between"""
    from latok_amd import batch
    rng = random.Random(7)
    ta = random_strings(rng, 12000, 0, 300, ALPHA)
    tb = random_strings(rng, 900, 0, 120, ALPHA)
    tc = random_strings(rng, 500, 0, 100, ALPHA)
    ar = _Arena(gpu)
    try:
        ea, eb, ec = (_expect(oracle, t, feats=False) for t in (ta, tb, tc))
        (ua, _, d_ua, d_oa), (ub, _, d_ub, d_ob), (uc, _, d_uc, d_oc) = (_resident(ar, t) for t in (ta, tb, tc))
        for leg in ("records", "result"):
            for _ in range(2):
                ja = _Job(ar, d_ua, d_oa, len(ta), ua.size, "offsets", np.int32)
                jc = _Job(ar, d_uc, d_oc, len(tc), uc.size, "spans", np.int32)
                jb = _Job(ar, d_ub, d_ob, len(tb), ub.size, "offsets", np.int32)
                if leg == "records":
                    jb.d_items, jb.cap = ja.d_items, ja.cap
                else:
                    jb.d_res = ja.d_res
                ja.submit()
                jc.submit()
                jb.submit()
                batch.flow_wait()
                _check(jb, eb, leg)
                _check(jc, ec, leg)
                if leg == "result":     # A's records and counts are its own; only the result words are B's
                    assert np.array_equal(ja.raw_items(ea["offs"].size), ea["offs"])
                    assert np.array_equal(ar.get(ja.d_counts, len(ta), np.int32), ea["o_counts"])
    finally:
        ar.free()


def test_interleaved_with_the_other_input_forms_in_one_flow(gpu, oracle):
    """code-point UTF-8 batches between UTF-32 and byte-space batches: every slot workspace serves all three in turn"""
    from latok_amd import _lib, batch
    rng = random.Random(2718)
    ar = _Arena(gpu)
    try:
        work = []
        for k in range(6):
            texts = random_strings(rng, 400 + 900 * k, 0, 60 + 50 * k, ALPHA)
            u8, boff, d_u8, d_boff = _resident(ar, texts)
            e = _expect(oracle, texts, feats=(k < 3))
            d_cps, d_row = ar.put(e["cps"]), ar.put(e["row"])
            jobs = [_Job(ar, d_u8, d_boff, len(texts), u8.size, f, np.int32) for f in ("mask", "offsets", "spans", "features")]
            d_m32, d_mb = ar.alloc((e["total"] + 63) // 64 * 8, POISON), ar.alloc((u8.size + 63) // 64 * 8, POISON)
            d_c32, d_o32, d_r32 = ar.alloc(len(texts) * 4), ar.alloc(e["total"] * 4), ar.alloc(16)
            work.append((texts, u8, boff, d_u8, d_boff, e, d_cps, d_row, jobs, d_m32, d_mb, d_c32, d_o32, d_r32))
        for _ in range(2):
            for texts, u8, boff, d_u8, d_boff, e, d_cps, d_row, jobs, d_m32, d_mb, d_c32, d_o32, d_r32 in work:
                jobs[0].submit()
                batch.flow_split_mask(d_cps, d_row, len(texts), e["total"], d_m32)
                jobs[1].submit()
                batch.flow_split_mask_utf8_bytes(d_u8, d_boff, len(texts), u8.size, d_mb)
                jobs[2].submit()
                batch.flow_split_offsets(d_cps, 4, d_row, len(texts), e["total"], d_c32, d_o32, e["total"], d_r32, dtype=np.int32)
                jobs[3].submit()
            batch.flow_wait()
            for texts, u8, boff, d_u8, d_boff, e, d_cps, d_row, jobs, d_m32, d_mb, d_c32, d_o32, d_r32 in work:
                for j in jobs:
                    _check(j, e, "interleaved")
                assert np.array_equal(ar.get(d_m32, e["bits"].size, np.uint64), e["bits"])
                assert np.array_equal(ar.get(d_mb, (u8.size + 63) // 64, np.uint64), batch.split_mask_utf8_bytes_csr(u8, boff))
                assert ar.get(d_r32, 2, np.int64).tolist() == [e["offs"].size, 0]
                assert np.array_equal(ar.get(d_o32, e["offs"].size, np.int32), e["offs"])
    finally:
        ar.free()


def test_two_contexts_at_once(gpu, oracle):
    from latok_amd import _lib, batch
    rng = random.Random(5)
    sets = [[random_strings(rng, 1500 + 500 * k, 0, 150, ALPHA) for k in range(3)] for _ in range(2)]
    wants = [[_expect(oracle, t, feats=False) for t in s] for s in sets]
    errors = []

    def worker(i):
        try:
            ctx = _lib.Context(0)
            with ctx:
                ar = _Arena(gpu)
                try:
                    for _ in range(3):
                        jobs = []
                        for texts, e in zip(sets[i], wants[i]):
                            u8, boff, d_u8, d_boff = _resident(ar, texts)
                            for f in ("mask", "offsets", "spans"):
                                j = _Job(ar, d_u8, d_boff, len(texts), u8.size, f, np.int32)
                                j.submit()
                                jobs.append((j, e))
                        batch.flow_wait()
                        for j, e in jobs:
                            _check(j, e, ("context", i))
                        ar.free()
                finally:
                    ar.free()
            ctx.destroy()
        except BaseException as exc:     # noqa: BLE001 -- reported by the main thread
            errors.append(repr(exc))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_a_slot_workspace_that_grows_mid_flow(gpu, oracle):
    """a fresh context: a small batch sizes the slot's buffers, a much larger one has to grow them (the flow is drained first),
    a small one follows; the per-slot lead / SPACE / packed-mask / row-offset / rule-code buffers grow with the rest"""
    from latok_amd import _lib, batch
    rng = random.Random(64)
    small = random_strings(rng, 40, 0, 50, ALPHA)
    big = random_strings(rng, 9000, 0, 400, ALPHA)
    es, eb = _expect(oracle, small), _expect(oracle, big)
    ctx = _lib.Context(0)
    with ctx:
        ar = _Arena(gpu)
        try:
            us, _, d_us, d_os = _resident(ar, small)
            ub, _, d_ub, d_ob = _resident(ar, big)
            assert ub.size > 20 * 65536
            for form in ("features", "spans", "offsets", "mask"):
                jobs = [(_Job(ar, d_us, d_os, len(small), us.size, form, np.int32), es), (_Job(ar, d_us, d_os, len(small), us.size, form, np.int64), es),
                        (_Job(ar, d_ub, d_ob, len(big), ub.size, form, np.int32), eb), (_Job(ar, d_us, d_os, len(small), us.size, form, np.int32), es),
                        (_Job(ar, d_ub, d_ob, len(big), ub.size, form, np.int64), eb)]
                for j, _ in jobs:
                    j.submit()
                batch.flow_wait()
                for j, e in jobs:
                    _check(j, e, ("grow", form))
        finally:
            ar.free()
    ctx.destroy()


def test_refused_arguments(gpu):
    from latok_amd import batch
    with pytest.raises(ValueError):
        batch.flow_split_offsets_utf8(0x1000, 0x2000, 3, 10, 0x3000, 0x4000, 10, None)          # NULL result words
    with pytest.raises(ValueError):
        batch.flow_split_offsets_utf8(0x1004, 0x2000, 3, 10, 0x3000, 0x4000, 10, 0x5000)        # misaligned bytes
    with pytest.raises(ValueError):
        batch.flow_split_mask_utf8(0x1000, 0x2000, 3, 10, 0x3000, 1, None, 0x5000)              # NULL row offsets
    with pytest.raises(ValueError):
        batch.flow_token_features_utf8(0x1000, 0x2000, 3, 10, 0x3000, 0x4000, None, 10, 0x5000)  # NULL feature sums


def test_c_example_flow_utf8_codepoints(gpu, oracle, tmp_path):
    """examples/flow_utf8_codepoints.c: a plain C caller submits two UTF-8 batches, reads the four result words after one wait,
    prints the oracle's code-point offsets of the well-formed batch and sends the malformed one through the blocking call."""
    import os
    import subprocess
    from conftest import ROOT
    from latok_amd import batch
    exe = str(tmp_path / "flow_utf8")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "flow_utf8_codepoints.c"),
                           "-L" + os.path.join(ROOT, "latok_amd"), "-llatok_hip", "-Wl,-rpath," + os.path.join(ROOT, "latok_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, timeout=120, check=True).stdout.decode("utf-8").splitlines()
    good = ["café 日本語 #tag", "", "🤓 me@x.org"]
    bad = [b"fine", b"a\x80\x80\x80\x80 stray continuation bytes"]
    want = ["batch 0: %d code points, well formed" % sum(map(len, good))]
    want += ["0.%d:" % i + "".join(" %d" % o for o in (oracle.split_offsets(t) if t else [])) for i, t in enumerate(good)]
    cps, row = batch.utf8_decode_csr(*batch.pack_utf8(bad))                       # what the staged decoder makes of the bytes
    want_cps, want_row, _ = utf8_ref.decode_batch(*batch.pack_utf8(bad))
    assert np.array_equal(cps, want_cps) and np.array_equal(row, want_row)
    decoded = [cps[row[i]:row[i + 1]].astype("<u4").tobytes().decode("utf-32-le", "surrogatepass") for i in range(len(bad))]
    want += ["batch 1: %d code points, malformed -> blocking call" % sum(b[0] & 0xC0 != 0x80 for b in [bytes([x]) for x in b"".join(bad)])]
    want += ["1.%d:" % i + "".join(" %d" % o for o in oracle.split_offsets(t)) for i, t in enumerate(decoded)]
    assert out == want
