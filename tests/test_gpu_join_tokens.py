"""Joined token text on the device (latok_join_tokens_utf8_bytes_batch / latok_flow_join_tokens_utf8_bytes, include/latok_hip.h).

The result is DEFINED by a call the parity tests already pin: row(s) = sep.join of the byte slices latok_token_spans_utf8_bytes_batch
reports for string s.  Every batch here is checked against that definition in full -- out_off, counts, every output byte, and guard
bytes behind out_off[n] that must stay untouched -- for the separators b" ", b"\\n", b"\\x00" and b"\\xff"; under the built-in tables
the rows are also what the oracle's tokenize() gives, and a golden file replays lines the real reference produced."""
import ctypes as C
import json
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ALPHABETS, GOLDEN, ROOT, RULE_SETS, random_strings
from helpers import span_strip_content as ssc

pytestmark = pytest.mark.gpu

SEPS = (b" ", b"\n", b"\x00", b"\xff")
POISON = 0xA5
GUARD = 64
JOIN_ROUTE = 5
ERR_CAP = 4             # bit of the flow's error word: the batch needs more than out_cap bytes
SOFT = [b"ab\xe6\x97 cd", b"\xc3 x", b"lone \xf0\x9f\x98", b"end\xe6", b"next starts ascii", b"\xe6\x97\xa5\xe6", b"\xf0", b"x\xc3"]
HARD = [b"a\x80\x80\x80\x80b", b"\xa9 starts with a continuation byte"]


def _enc(texts):
    return [t.encode("utf-8", "surrogatepass") for t in texts]


def _slices(blobs):
    """per string the token slices the spans call defines, and its counts"""
    from latok_amd import batch
    u8, boff = batch.pack_utf8(blobs)
    counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
    out, k = [], 0
    for blob, n in zip(blobs, counts.tolist()):
        out.append([blob[a:b] for a, b in spans[k:k + n].tolist()])
        k += n
    return u8, boff, counts, out


def _join_host(lib, u8, boff, sep, cap=None, counts_dt=np.int64, out=True, total=None):
    """the blocking call with host pointers -> (rc, n, out incl. guard bytes, out_off, counts)"""
    from latok_amd import _lib
    n_str = boff.size - 1
    total = (int(boff[-1]) if n_str > 0 else 0) if total is None else total
    cap = 2 * max(int(boff[-1]) if n_str > 0 else 0, 0) if cap is None else cap
    buf = np.full(cap + GUARD, POISON, np.uint8)
    off = np.full(n_str + 1, -7, np.int64)
    counts = np.full(n_str, -7, counts_dt)
    n = C.c_int64(-1)
    rc = lib.latok_join_tokens_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, sep[0], buf.ctypes.data if out else None, cap,
                                                off.ctypes.data, counts.ctypes.data, C.byref(n),
                                                _lib.OUT_INT32 if counts_dt == np.int32 else 0, None)
    return rc, n.value, buf, off, counts


def _check_definition(lib, blobs, what, seps=SEPS, oracle=None, texts=None):
    from latok_amd import _lib
    u8, boff, counts, toks = _slices(blobs)
    for sep in seps:
        rows = [sep.join(t) for t in toks]
        want = b"".join(rows)
        want_off = np.zeros(len(blobs) + 1, np.int64)
        np.cumsum([len(r) for r in rows], out=want_off[1:])
        rc, n, buf, off, got_counts = _join_host(lib, u8, boff, sep)
        assert rc == 0, (what, sep, _lib.last_error())
        assert lib.latok_debug_last_route() == JOIN_ROUTE or int(boff[-1]) == 0
        assert n == len(want), (what, sep, n, len(want))
        assert np.array_equal(off, want_off), (what, sep, "out_off", int(np.nonzero(off != want_off)[0][0]))
        assert np.array_equal(got_counts, counts), (what, sep, "counts")
        got = buf[:n].tobytes()
        if got != want:
            bad = next(i for i in range(n) if got[i] != want[i])
            s = int(np.searchsorted(want_off, bad, side="right")) - 1
            raise AssertionError((what, sep, "byte", bad, "string", s, got[max(bad - 20, 0):bad + 20], want[max(bad - 20, 0):bad + 20]))
        assert (buf[n:] == POISON).all(), (what, sep, "guard bytes")
        assert n <= 2 * int(boff[-1] if boff.size > 1 else 0)
    if oracle is not None:   # built-in tables: the reference's own line (sep = one space, the rows of the last check differ only in sep)
        rows = [b" ".join(t) for t in toks]
        for text, row in zip(texts, rows):
            exp = " ".join(oracle.tokenize(text)).encode("utf-8", "surrogatepass") if text != "" else b""
            assert row == exp, (what, text[:80])
            if text.strip() == "":
                assert row == b""
    return u8, boff, counts, toks


# ---- random content --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet", sorted(ALPHABETS))
def test_random_strings_at_three_sizes(gpu, oracle, alphabet):
    rng = random.Random(zlib.crc32(alphabet.encode()))
    alpha = ALPHABETS[alphabet]
    sizes = ((random_strings(rng, 200, 0, 12, alpha), "one tile"),                 # (cut below to what fits one tile)
             (random_strings(rng, 3000, 0, 40, alpha), "<= 262144 bytes"),
             (random_strings(rng, 24000, 0, 120, alpha) + ["".join(rng.choice(alpha) for _ in range(150000))], "several hundred tiles"))
    for texts, what in sizes:
        blobs = _enc(texts)
        total = sum(map(len, blobs))
        if what == "one tile":
            while total > 4096:
                blobs.pop()
                texts.pop()
                total = sum(map(len, blobs))
            assert len(blobs) < 512 and total <= 4096
        elif what == "<= 262144 bytes":
            assert 4096 < total <= 262144
        else:
            assert total > 300 * 4096
        _check_definition(gpu, blobs, (alphabet, what), oracle=oracle if total <= 262144 else None, texts=texts)


@pytest.mark.parametrize("name", sorted(RULE_SETS))
def test_runtime_rule_tables(gpu, name):
    from latok_amd import batch
    rng = random.Random(77)
    texts = random_strings(rng, 2500, 0, 150, ALPHABETS["mixed"]) + ["   ", "", " a ", "　x　"]
    batch.set_rules(*RULE_SETS[name])
    try:
        _check_definition(gpu, _enc(texts), ("rules", name))
        _check_definition(gpu, _enc(texts[:40]), ("rules small", name))
    finally:
        batch.reset_rules()


@pytest.mark.parametrize("table", sorted(ssc.TABLES))
@pytest.mark.parametrize("size", ssc.SIZES)
def test_tables_that_leave_whitespace_inside_tokens(gpu, table, size):
    """interior whitespace is copied, only the two ends of a token are stripped; long whitespace in front of, inside and behind tokens"""
    from latok_amd import batch
    batch.set_rules(*ssc.TABLES[table])
    try:
        for i, texts in enumerate(ssc.content(table, size, "bytes", "full")):
            _check_definition(gpu, _enc(texts), (table, size, "ABCD"[i]))
    finally:
        batch.reset_rules()


# ---- edges -----------------------------------------------------------------------------------------------------------------
def _edge_batch(at):
    """strings whose starts and whose tokens' ends fall on at - 1, at, at + 1 bytes of the packed batch, and a 4-byte char that
    straddles `at` at a token's end"""
    blobs, pos = [], 0

    def pad_to(p):
        nonlocal pos
        assert p >= pos, (p, pos)
        while pos < p:
            n = min(p - pos, 61)
            blobs.append((b"w" * (n - 1) + b" ") if n > 1 else b"x")
            pos += n

    base = at
    for d in (-1, 0, 1):                         # a string starts at at + d, its first token ends 3 bytes later
        pad_to(base + d)
        blobs.append(b"abc, de")
        pos += 7
        base += 4096 if at % 4096 == 0 else 64
    for d in (-1, 0, 1):                         # a token ends at base + d (the comma is the next token)
        s = b"  lead tok"
        pad_to(base + d - len(s))
        blobs.append(s + b", tail ")
        pos += len(s) + 7
        base += 4096 if at % 4096 == 0 else 64
    for k in (1, 2, 3):                          # a 4-byte char ends a token, k of its bytes in front of the edge
        s = b"word" + "🤓".encode()
        pad_to(base + (4 - k) - len(s))
        blobs.append(s + b" next")
        pos += len(s) + 5
        base += 4096 if at % 4096 == 0 else 64
    return blobs


def test_word_and_tile_edges(gpu, oracle):
    for at in (64, 128, 64 * 63, 4096, 8192, 4096 * 5):
        blobs = _edge_batch(at)
        texts = [b.decode() for b in blobs]
        _check_definition(gpu, blobs, ("edges", at), oracle=oracle, texts=texts)


def test_output_runs_begin_at_every_alignment(gpu):
    """tile t's output run begins where the tiles before it end: a first string of 1 .. 8 kept bytes in front of several tiles"""
    for k in range(1, 9):
        blobs = [b"x" * k + b" " * (4096 - k)] + [b"ab cd, ef " * 500, b"", b"tail"]
        _check_definition(gpu, blobs, ("alignment", k))


def test_tiles_of_one_byte_tokens_reach_the_size_bound(gpu, oracle):
    """every byte a token of its own: two output bytes per input byte, 8192 items in a tile -- the only bound there is"""
    blobs = [b"a,b," * 5000, b",", b";.!?" * 3000, b"x"]
    u8, boff, counts, toks = _check_definition(gpu, blobs, "one-byte tokens", oracle=oracle, texts=[b.decode() for b in blobs])
    rc, n, buf, off, c = _join_host(gpu, u8, boff, b" ")
    assert rc == 0 and n == 2 * int(boff[-1]) - len(blobs) and c.tolist() == [20000, 1, 12000, 1]


def test_empty_strings_whitespace_and_nothing(gpu):
    from latok_amd import batch
    body = [b"some text, here", b"more"]
    for blobs in ([b""] * 70 + body + [b""] * 130 + body + [b""] * 70, [b""] * 5, [b"", b"x", b""]):
        _check_definition(gpu, blobs, "runs of empty strings")
    ws = [b"   ", b"\t\n", "　　".encode(), b" " * 5000, b""] * 3
    u8, boff, counts, toks = _check_definition(gpu, ws, "all whitespace")
    rc, n, buf, off, c = _join_host(gpu, u8, boff, b" ")
    assert rc == 0 and n == 0 and not off.any() and not c.any()
    # n_str = 0
    rc, n, buf, off, c = _join_host(gpu, np.zeros(0, np.uint8), np.zeros(1, np.int64), b" ")
    assert rc == 0 and n == 0 and off[0] == 0 and (buf == POISON).all()
    assert batch.join_tokens_utf8_batch([]) == [] and batch.join_tokens_batch([""]) == [""]


def test_long_tokens_and_long_whitespace(gpu):
    from latok_amd import batch
    M = 1 << 20
    _check_definition(gpu, [b"a" * M], "one 1 M-char token")
    _check_definition(gpu, [b"xy", b"q" * M, b"ab cd"], "1 M-char token between strings")
    _check_definition(gpu, [b" " * M + b"tok, end", b"next one"], "1 M bytes of whitespace in front of a token")
    # under a table that splits at upper-case letters only: whitespace inside tokens, a token whose only non-SPACE byte is its
    # last, 1 M bytes of whitespace between a string's start and its first kept token and inside one token
    batch.set_rules(*ssc.TABLES["UPPER_ONLY"])
    try:
        _check_definition(gpu, [b" " * M + b"x", b"Ab" + b" " * 70000 + b"c Def"], "only non-SPACE byte is the last")
        _check_definition(gpu, [b"Aa", b" " * M + b"Bcd  e" + b" " * 9000 + b"Fg " + b" " * M, b" Hi"], "whitespace prefix of a string")
        _check_definition(gpu, [b"A" + b" " * M + b"b C"], "1 M bytes of whitespace inside a token")
    finally:
        batch.reset_rules()


def test_malformed_bytes_follow_the_spans_call(gpu):
    rng = random.Random(5)
    body = _enc(random_strings(rng, 3000, 0, 120, ALPHABETS["mixed"]))
    _check_definition(gpu, body[:1500] + SOFT + body[1500:] + SOFT, "soft malformed")
    _check_definition(gpu, body[:700] + HARD + SOFT + body[700:] + HARD, "hard malformed")
    _check_definition(gpu, SOFT + HARD, "small malformed batch")


# ---- capacity --------------------------------------------------------------------------------------------------------------
def test_capacity_protocol(gpu):
    from latok_amd import _lib
    rng = random.Random(9)
    blobs = _enc(random_strings(rng, 900, 0, 90, ALPHABETS["mixed"]))
    u8, boff, counts, toks = _slices(blobs)
    rows = [b" ".join(t) for t in toks]
    want = b"".join(rows)
    want_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    need = len(want)
    # size query
    rc, n, buf, off, c = _join_host(gpu, u8, boff, b" ", cap=0, out=False)
    assert rc == _lib.ERR_INVALID and n == need and np.array_equal(off, want_off) and np.array_equal(c, counts)
    # one byte short: nothing written, everything else valid
    rc, n, buf, off, c = _join_host(gpu, u8, boff, b" ", cap=need - 1)
    assert rc == _lib.ERR_INVALID and "capacity" in _lib.last_error() and n == need
    assert (buf == POISON).all() and np.array_equal(off, want_off) and np.array_equal(c, counts)
    # exact
    rc, n, buf, off, c = _join_host(gpu, u8, boff, b" ", cap=need, counts_dt=np.int32)
    assert rc == 0 and n == need and buf[:need].tobytes() == want and (buf[need:] == POISON).all()
    assert c.dtype == np.int32 and np.array_equal(c, counts) and np.array_equal(off, want_off)
    # a NULL buffer with a capacity is refused; so is a separator that is no byte
    rc, n, buf, off, c = _join_host(gpu, u8, boff, b" ", cap=need, out=False)
    assert rc == _lib.ERR_INVALID and "out_bytes" in _lib.last_error()
    n_out = C.c_int64(0)
    for sep in (-1, 256):
        rc = gpu.latok_join_tokens_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, boff.size - 1, -1, sep, buf.ctypes.data, need,
                                                    off.ctypes.data, None, C.byref(n_out), 0, None)
        assert rc == _lib.ERR_INVALID and "sep" in _lib.last_error()
    rc = gpu.latok_join_tokens_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, boff.size - 1, -1, 32, buf.ctypes.data, need,
                                                off.ctypes.data, None, C.byref(n_out), 64, None)
    assert rc == _lib.ERR_INVALID and "unknown flag" in _lib.last_error()
    # counts are optional; total_bytes = -1 is resolved from byte_off
    off2 = np.zeros_like(off)
    rc = gpu.latok_join_tokens_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, boff.size - 1, -1, 32, buf.ctypes.data, need,
                                                off2.ctypes.data, None, C.byref(n_out), 0, None)
    assert rc == 0 and n_out.value == need and np.array_equal(off2, want_off)


# ---- pointer modes ---------------------------------------------------------------------------------------------------------
class _Dev:
    """a batch resident on the device + poisoned output buffers"""

    def __init__(self, lib, u8, boff, cap, counts_dt=np.int64, shift=0):
        from latok_amd import _lib
        self.lib, self.n_str, self.total, self.cap, self.dt = lib, boff.size - 1, int(boff[-1]), cap, np.dtype(counts_dt)
        sizes = (u8.nbytes + 128, boff.nbytes, cap + GUARD, boff.nbytes, self.n_str * 8 + 16, 64)
        self.ptrs = [lib.latok_dev_alloc(s) for s in sizes]
        assert all(self.ptrs)
        self.u8, self.boff, self.out, self.off, self.counts, self.res = self.ptrs
        self.u8 += shift
        _lib.check(lib.latok_memcpy_h2d(self.u8, u8.ctypes.data, u8.nbytes))
        _lib.check(lib.latok_memcpy_h2d(self.boff, boff.ctypes.data, boff.nbytes))
        for p, s in zip(self.ptrs[2:], sizes[2:]):
            _lib.check(lib.latok_memset_dev(p, POISON, s))
        _lib.check(lib.latok_sync())

    def read(self):
        from latok_amd import _lib
        buf, off = np.empty(self.cap + GUARD, np.uint8), np.empty(self.n_str + 1, np.int64)
        counts, res = np.empty(self.n_str, self.dt), np.empty(2, np.int64)
        for a, p in ((buf, self.out), (off, self.off), (counts, self.counts), (res, self.res)):
            if a.nbytes:
                _lib.check(self.lib.latok_memcpy_d2h(a.ctypes.data, p, a.nbytes))
        return buf, off, counts, res

    def free(self):
        for p in self.ptrs:
            self.lib.latok_dev_free(p)


def test_device_pointers_equal_host_pointers_and_a_second_context(gpu):
    from latok_amd import _lib
    rng = random.Random(21)
    blobs = _enc(random_strings(rng, 4000, 0, 200, ALPHABETS["mixed"]))
    u8, boff, counts, toks = _slices(blobs)
    rc, need, want_buf, want_off, want_counts = _join_host(gpu, u8, boff, b"\n")
    assert rc == 0
    d = _Dev(gpu, u8, boff, need, np.int32)
    try:
        n = C.c_int64(-1)
        flags = _lib.DEVICE_PTRS | _lib.OUT_INT32
        rc = gpu.latok_join_tokens_utf8_bytes_batch(d.u8, d.boff, d.n_str, -1, 10, d.out, need, d.off, d.counts, C.byref(n), flags, None)
        assert rc == 0 and n.value == need, _lib.last_error()
        buf, off, c, _ = d.read()
        assert buf[:need].tobytes() == want_buf[:need].tobytes() and (buf[need:] == POISON).all()
        assert np.array_equal(off, want_off) and np.array_equal(c, want_counts)
        # an unaligned device input is refused
        rc = gpu.latok_join_tokens_utf8_bytes_batch(d.u8 + 4, d.boff, d.n_str, d.total, 10, d.out, need, d.off, d.counts, C.byref(n), flags, None)
        assert rc == _lib.ERR_INVALID and "16-byte aligned" in _lib.last_error()
    finally:
        d.free()
    with _lib.Context(0):
        rc, n2, buf2, off2, c2 = _join_host(gpu, u8, boff, b"\n")
        assert rc == 0 and n2 == need and buf2.tobytes() == want_buf.tobytes() and np.array_equal(off2, want_off) and np.array_equal(c2, want_counts)


# ---- the flow --------------------------------------------------------------------------------------------------------------
def test_flow_batches_alternating_over_two_output_buffers(gpu):
    from latok_amd import _lib, batch
    rng = random.Random(33)
    batches = [_enc(random_strings(rng, n, 0, hi, ALPHABETS[a])) for n, hi, a in ((3000, 150, "mixed"), (50, 30, "words"), (6000, 90, "bmp"),
                                                                                 (2000, 300, "latin1"))]
    packed = [batch.pack_utf8(b) for b in batches]
    want = [_join_host(gpu, u8, boff, b"\n") for u8, boff in packed]
    cap = max(w[1] for w in want)
    devs = [_Dev(gpu, u8, boff, cap) for u8, boff in packed]
    outs = [gpu.latok_dev_alloc(cap + GUARD) for _ in range(2)]
    try:
        for first in (0, 2):                # two batches in flight at a time, one per output buffer; nothing waits in between
            pair = devs[first:first + 2]
            for i, d in enumerate(pair):
                batch.flow_join_tokens_utf8_bytes(d.u8, d.boff, d.n_str, d.total if i else -1, outs[i], cap, d.off, d.counts, d.res, sep=b"\n")
            batch.flow_wait()
            for i, d in enumerate(pair):
                rc, n, wbuf, woff, wc = want[first + i]
                _, off, c, res = d.read()
                assert res.tolist() == [n, 0], (first + i, res)
                assert np.array_equal(off, woff) and np.array_equal(c, wc), first + i
                got = np.empty(cap + GUARD, np.uint8)
                _lib.check(gpu.latok_memcpy_d2h(got.ctypes.data, outs[i], got.nbytes))
                assert got[:n].tobytes() == wbuf[:n].tobytes(), first + i
        # resubmission into the same output buffer with no wait between: the second result wins
        a, b = devs[0], devs[2]
        batch.flow_join_tokens_utf8_bytes(a.u8, a.boff, a.n_str, a.total, outs[0], cap, a.off, a.counts, a.res, sep=b"\n")
        batch.flow_join_tokens_utf8_bytes(b.u8, b.boff, b.n_str, b.total, outs[0], cap, b.off, b.counts, b.res, sep=b" ")
        batch.flow_wait()
        got = np.empty(cap, np.uint8)
        _lib.check(gpu.latok_memcpy_d2h(got.ctypes.data, outs[0], cap))
        rc, n_sp, buf_sp, _, _ = _join_host(gpu, *packed[2], b" ")
        assert got[:n_sp].tobytes() == buf_sp[:n_sp].tobytes()
        # a batch whose capacity is too small leaves its output untouched and reports the needed size and the error bit
        d = devs[0]
        _lib.check(gpu.latok_memset_dev(outs[1], POISON, cap + GUARD))
        _lib.check(gpu.latok_sync())
        batch.flow_join_tokens_utf8_bytes(d.u8, d.boff, d.n_str, d.total, outs[1], want[0][1] - 1, d.off, None, d.res, sep=b"\n")
        batch.flow_wait()
        got = np.empty(cap + GUARD, np.uint8)
        _lib.check(gpu.latok_memcpy_d2h(got.ctypes.data, outs[1], got.nbytes))
        _, off, _, res = d.read()
        assert (got == POISON).all() and res.tolist() == [want[0][1], ERR_CAP] and np.array_equal(off, want[0][3])
        # an "unbounded" capacity works like the exact one
        batch.flow_join_tokens_utf8_bytes(d.u8, d.boff, d.n_str, d.total, outs[1], 1 << 62, d.off, d.counts, d.res, sep=b"\n")
        batch.flow_wait()
        _lib.check(gpu.latok_memcpy_d2h(got.ctypes.data, outs[1], got.nbytes))
        n = want[0][1]
        assert got[:n].tobytes() == want[0][2][:n].tobytes() and d.read()[3].tolist() == [n, 0]
        # an empty batch in the flow: zero rows, zero total
        e = _Dev(gpu, np.zeros(0, np.uint8), np.zeros(4, np.int64), 16)
        try:
            batch.flow_join_tokens_utf8_bytes(e.u8, e.boff, 3, 0, e.out, 16, e.off, e.counts, e.res)
            batch.flow_wait()
            buf, off, c, res = e.read()
            assert res.tolist() == [0, 0] and not off.any() and not c.any() and (buf == POISON).all()
        finally:
            e.free()
    finally:
        for d in devs:
            d.free()
        for p in outs:
            gpu.latok_dev_free(p)


# ---- Python surface, golden, example ---------------------------------------------------------------------------------------
def test_python_wrappers(gpu, oracle):
    from latok_amd import batch
    rng = random.Random(3)
    texts = random_strings(rng, 500, 0, 80, ALPHABETS["mixed"]) + ["", "   ", "x", "\ud800 lone", "a,b"]
    blobs = _enc(texts)
    want = [b" ".join(t) for t in batch.tokenize_utf8_batch(blobs)]
    assert batch.join_tokens_utf8_batch(blobs) == want
    assert batch.join_tokens_utf8_batch(blobs, b"\x00") == [b"\x00".join(t) for t in batch.tokenize_utf8_batch(blobs)]
    assert batch.join_tokens_batch(texts) == [w.decode("utf-8", "surrogatepass") for w in want]
    plain = [t for t in texts if "\ud800" not in t]
    assert batch.join_tokens_batch(plain, "\n") == ["\n".join(oracle.tokenize(t)) if t.strip() else "" for t in plain]
    assert batch.join_tokens_batch(["a,b"]) == ["a , b"]
    u8, boff = batch.pack_utf8(blobs)
    out, off, counts = batch.join_tokens_utf8_csr(u8, boff, b" ", dtype=np.int32)
    assert out.tobytes() == b"".join(want) and off.dtype == np.int64 and counts.dtype == np.int32
    assert [out[a:b].tobytes() for a, b in zip(off[:-1], off[1:])] == want
    assert np.array_equal(counts, [len(t) for t in batch.tokenize_utf8_batch(blobs)])


def test_golden_lines_of_the_real_reference(gpu):
    from latok_amd import batch
    g = json.load(open(os.path.join(GOLDEN, "join_tokens.json")))
    items = json.load(open(os.path.join(GOLDEN, "ref_strings.json")))["items"]
    texts = ["".join(map(chr, it["cps"])) for it in items] + [json.load(open(os.path.join(GOLDEN, "c1_paragraph.json")))["text"]]
    assert len(texts) == len(g["rows"]) and g["sep"] == " "
    want = ["" if r is None else r for r in g["rows"]]
    assert batch.join_tokens_batch(texts, " ") == want
    for t, w in zip(texts, want):   # one string per call as well
        assert batch.join_tokens_batch([t]) == [w]


def test_c_example(gpu, tmp_path):
    exe = str(tmp_path / "join_tokens_utf8")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "join_tokens_utf8.c"),
                           "-L" + os.path.join(ROOT, "latok_amd"), "-llatok_hip", "-Wl,-rpath," + os.path.join(ROOT, "latok_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "0 (12 tokens): This is a #test ! Testing , Testing , 1 2 3"
    assert lines[2] == "2 (0 tokens): " and lines[3] == "3 (0 tokens): "
    assert lines[4].startswith("4 (") and lines[4].endswith("🤓")
