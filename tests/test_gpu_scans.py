"""The two device-wide exclusive scans of int64 counts, at every block and look-back edge: k_scan_chained (compact_kernels.hip: 4096
entries per workgroup, a look-back of 64 predecessors per round over published words of a 44-bit value, a flag and an 18-bit launch
epoch) and launch_exclusive_scan (aux_kernels.hip: one k_scan_small, or k_scan_local + k_scan_totals + k_scan_add).

latok_debug_scan runs each scan exactly as the calls run it on an array the test supplies; tests/helpers/scan_cases.py builds the
arrays from the limits the library reports and the expectation is np.cumsum in int64.  Every result is compared in full and exactly:
the entries, the total, the scan's error flag, the poisoned guard words behind the output and the input itself.  The public calls
follow at the smallest batches whose row scans take a second look-back round; they depend on a fixture that first verifies the scans
through the hook, whose results only land in the test's own buffers -- a wrong scan result would feed scatter kernels that index with it.

The epoch tests leave stale words of the same epoch and slot in the chain array; they cannot force the interleaving in which a
workgroup would read one."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_ngram_counts as ng
import test_gpu_term_counts as tc
import test_gpu_wordpiece as wpt
from helpers import scan_cases as sc

pytestmark = pytest.mark.gpu

GUARD = 16
POISON_64 = np.int64(-0x5A5A5A5A5A5A5A5B)          # 0xA5 in every byte
CHAINED, THREE_LAUNCH = 0, 1
LIM = sc.limits()
EPOCH_MASK = (1 << LIM.epoch_bits) - 1


class Scanner:
    """device buffers of the hook on the current context, grown as needed: the input, the output with GUARD words behind it, the units word"""

    def __init__(self, lib):
        from latok_amd import _lib
        self.lib, self.check, self.cap, self.ptrs = lib, _lib.check, 0, []
        fn = lib.latok_debug_scan
        fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)]

    def _reserve(self, n):
        if n > self.cap:
            self.close()
            self.ptrs = [self.lib.latok_dev_alloc(8 * n), self.lib.latok_dev_alloc(8 * (n + GUARD)), self.lib.latok_dev_alloc(64)]
            assert all(self.ptrs)
            self.cap = n

    def close(self):
        for p in self.ptrs:
            self.lib.latok_dev_free(p)
        self.ptrs, self.cap = [], 0

    def run(self, which, v, units=None):
        """-> (out[n + GUARD], total, flag, the input as the device holds it afterwards)"""
        n = v.size
        self._reserve(n)
        d_in, d_out, d_units = self.ptrs
        self.check(self.lib.latok_memcpy_h2d(d_in, v.ctypes.data, 8 * n))
        self.check(self.lib.latok_memset_dev(d_out, 0xA5, 8 * (n + GUARD)))
        if units is not None:
            word = np.array([units], np.int64)
            self.check(self.lib.latok_memcpy_h2d(d_units, word.ctypes.data, 8))
        total, flag = C.c_int64(-3), C.c_int(-3)
        self.check(self.lib.latok_debug_scan(which, d_in, n, d_out, d_units if units is not None else None, C.byref(total), C.byref(flag)))
        out, back = np.empty(n + GUARD, np.int64), np.empty(n, np.int64)
        self.check(self.lib.latok_memcpy_d2h(out.ctypes.data, d_out, out.nbytes))
        self.check(self.lib.latok_memcpy_d2h(back.ctypes.data, d_in, back.nbytes))
        return out, total.value, flag.value, back

    def verify(self, which, v, what, units=None, real=None):
        """one scan, compared in full: entries up to the real size, the total, the flag, everything behind the real size, the input"""
        want, want_total = sc.expect(v, real)
        out, total, flag, back = self.run(which, v, units)
        real = v.size if real is None else real
        assert flag == 0, (what, "flag", flag)
        if not np.array_equal(out[:real], want):
            k = int(np.flatnonzero(out[:real] != want)[0])
            raise AssertionError((what, "entry", k, "of", real, "got", int(out[k]), "want", int(want[k]), "wrong:", int((out[:real] != want).sum())))
        assert total == want_total, (what, "total", total, want_total)
        assert (out[real:] == POISON_64).all(), (what, "written behind the scan's size", int(np.flatnonzero(out[real:] != POISON_64)[0]) + real)
        assert np.array_equal(back, v), (what, "the input changed")


@pytest.fixture(scope="module")
def scanner(gpu):
    s = Scanner(gpu)
    yield s
    s.close()


def _set_epoch(lib, epoch):
    lib.latok_debug_set_scan_epoch.restype, lib.latok_debug_set_scan_epoch.argtypes = C.c_int, [C.c_uint]
    assert lib.latok_debug_set_scan_epoch(epoch) == 0


# ---- 1. every length with every pattern that fits it -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,edge", sc.chained_lengths(LIM), ids=lambda x: str(x).replace(" ", "_"))
def test_chained_scan_at_every_length(scanner, n, edge):
    for name, v in sc.cases(n, n % 1000, LIM.chain_chunk, LIM.lookback, LIM.value_bits):
        scanner.verify(CHAINED, v, (edge, n, name))


@pytest.mark.parametrize("n,edge", sc.three_launch_lengths(LIM), ids=lambda x: str(x).replace(" ", "_"))
def test_three_launch_scan_at_every_length(scanner, n, edge):
    for name, v in sc.cases(n, n % 1000, LIM.scan_chunk, 0, LIM.value_bits):
        scanner.verify(THREE_LAUNCH, v, (edge, n, name))


def test_hook_refuses_an_empty_scan(scanner):
    from latok_amd import _lib
    scanner._reserve(8)
    total, flag = C.c_int64(0), C.c_int(0)
    for n in (0, -1):
        for which in (CHAINED, THREE_LAUNCH):
            assert scanner.lib.latok_debug_scan(which, scanner.ptrs[0], n, scanner.ptrs[1], None, C.byref(total), C.byref(flag)) == _lib.ERR_INVALID


# ---- 2. the device-sized chained scan: surplus workgroups behind a multi-workgroup real size ----------------------------------------------
def test_device_sized_chained_scan(scanner):
    n, reals = sc.device_sized_cases(LIM)
    tile = sc.tile_units()
    for k, pattern in enumerate(("mod7", "wide")):
        v = sc.values(pattern, n, 40 + k, LIM.chain_chunk, LIM.lookback, LIM.value_bits)
        for real in reals:
            # ceil(units / kTile) entries are real: the smallest and the largest unit count of that size, and one far beyond the grid
            for units in sorted({max(real * tile - tile + 1, 0), real * tile} | ({(n + 5) * tile} if real == n else set())):
                scanner.verify(CHAINED, v, ("device-sized", pattern, real, units), units=units, real=real)
    scanner.verify(CHAINED, v, ("device-sized", "negative word"), units=-5, real=0)
    scanner.verify(CHAINED, v, ("host-sized after device-sized",))


# ---- 3. epoch and state, on a fresh context ------------------------------------------------------------------------------------------
def test_epoch_wrap_and_state_on_a_fresh_context(gpu):
    from latok_amd import _lib
    c, w = LIM.chain_chunk, LIM.lookback
    big, small = (2 * w + 2) * c + 3, 2 * c + 1
    a, b = (sc.values(p, big, 7, c, w, LIM.value_bits) for p in ("mod7", "sparse"))
    b[::c] += 3                                                          # (no chunk total of B equals A's: a stale word cannot pass for a fresh one)
    small_v = sc.values("mod7", small, 8, c, w, LIM.value_bits)
    ctx = _lib.Context(_lib.default_device())
    try:
        with ctx:
            s = Scanner(gpu)
            try:
                # a context whose first scan has 2 workgroups grows to 130: the chain array is re-allocated, its state cleared
                s.verify(CHAINED, small_v[:c + 1], ("first scan of the context", 2))
                for k in range(3):                                       # (the new array starts at epoch 1) epochs 1 to 3: A's words in every slot
                    s.verify(CHAINED, a, ("A", k))
                _set_epoch(gpu, EPOCH_MASK - 2)
                for k in range(6):                                       # B across the wrap: its fifth run is on epoch 3 again, over A's slots
                    s.verify(CHAINED, b, ("B across the wrap", k))
                for k, v in enumerate((a, small_v, b, small_v, a)):      # alternating sizes on consecutive epochs
                    s.verify(CHAINED, v, ("alternating sizes", k))
                for start in range(EPOCH_MASK - 3, EPOCH_MASK + 1):
                    # (rewinding the epoch is sound here: the last run before it was a full-size A on an epoch above 2, so no slot
                    # holds a word of epoch 2 when A runs on it)
                    _set_epoch(gpu, 1)
                    s.verify(CHAINED, a, ("A on epoch 2", hex(start)))   # every slot holds a word of A with epoch 2 ...
                    _set_epoch(gpu, start)
                    for k, v in enumerate((small_v, b, b, b, b, a)):     # ... and whatever the start, the run that comes to epoch 2 again is a B
                        s.verify(CHAINED, v, ("wrap from", hex(start), k))
                s.verify(THREE_LAUNCH, b, ("the other scan on the same context",))
            finally:
                s.close()
    finally:
        ctx.destroy()


# ---- 4. the public calls at the smallest batches whose row scans take a second look-back round ------------------------------------------
@pytest.fixture(scope="module")
def scans_verified(scanner):
    """the public-call tests run only behind scans that the hook has shown to be right at their sizes"""
    c, w = LIM.chain_chunk, LIM.lookback
    for n in ((w + 1) * c + 1, (w + 2) * c + 1):
        for pattern in ("sparse", "mod7"):
            scanner.verify(CHAINED, sc.values(pattern, n, 3, c, w, LIM.value_bits), ("before the public calls", n, pattern))
    return True


ROW_PATTERNS = [b"", b"ab", b"ab cd", b"ab ab", b"zz", b"cd zz ab"]     # empty, one known word, two words, a repeated word, one unknown word, three
WORDS = [b"ab", b"cd", b"ab cd", b"ab ab", b"zz ab"]
SAMPLE = 2000


@functools.lru_cache(maxsize=None)
def _row_batch(n_str):
    """n_str strings drawn from ROW_PATTERNS, with runs of empty strings -> (pattern index per string, utf8, byte_off)"""
    from latok_amd import batch
    rng = np.random.default_rng(n_str)
    pat = rng.integers(0, len(ROW_PATTERNS), n_str)
    pat *= np.repeat(rng.random((n_str + 52) // 53) < 0.7, 53)[:n_str]
    pat[:len(ROW_PATTERNS)] = np.arange(len(ROW_PATTERNS))
    u8, boff = batch.pack_utf8([ROW_PATTERNS[k] for k in pat.tolist()])
    return pat, u8, boff


def _expand(table, pat):
    """the CSR of a batch from the CSR of its patterns: (indptr, indices, data, oov)"""
    indptr5, indices5, data5, oov5 = table
    d = np.diff(indptr5)[pat]
    indptr = np.zeros(pat.size + 1, np.int64)
    np.cumsum(d, out=indptr[1:])
    src = np.repeat(indptr5[:-1][pat], d) + (np.arange(int(indptr[-1])) - np.repeat(indptr[:-1], d))
    return indptr, indices5[src], data5[src], (oov5[pat] if oov5 is not None else None)


def _rows_call(gpu, n_str, want_fn, call, has_oov, dtypes, repeat=1):
    """one call family on the batch of n_str pattern rows, checked in full.  want_fn(token rows) -> ((indptr, indices, data[, oov]), items per
    row) is the existing definition; call(u8, boff, cap, dtype) -> (rc, nnz, items, _Out) one blocking call with guard bands"""
    from latok_amd import _lib, batch
    pat, u8, boff = _row_batch(n_str)
    u5, b5 = batch.pack_utf8(ROW_PATTERNS)
    rows5 = tc._rows_of_slices(u5, b5)
    want5, items5 = want_fn(rows5)
    table = (want5[0], want5[1], want5[2], want5[3] if has_oov else None)
    # the patterns against the definition, on a sample of the same batch
    rows_s = tc._rows_of_slices(u8[:boff[SAMPLE]], boff[:SAMPLE + 1])
    want_s, items_s = want_fn(rows_s)
    got_s = _expand(table, pat[:SAMPLE])
    assert all(np.array_equal(x, y) for x, y in zip(got_s[:3], want_s[:3])) and (not has_oov or np.array_equal(got_s[3], want_s[3]))
    assert np.array_equal(items5[pat[:SAMPLE]], items_s)
    indptr, indices, data, oov = _expand(table, pat)
    nnz, n_items = int(indptr[-1]), int(items5[pat].sum())
    for dt in dtypes:
        for k in range(repeat):
            rc, got_nnz, got_items, o = call(u8, boff, nnz, dt)
            what = (n_str, dt.__name__, k)
            assert rc == 0, (what, _lib.last_error())
            assert (got_nnz, got_items) == (nnz, n_items), (what, got_nnz, nnz, got_items, n_items)
            assert o.indptr.dtype == dt and np.array_equal(o.indptr[:n_str + 1], indptr), (what, "indptr")
            assert (o.indptr[n_str + 1:] == -7).all(), (what, "guard words behind indptr")
            assert np.array_equal(o.indices[:nnz], indices) and np.array_equal(o.data[:nnz], data), (what, "entries")
            assert (o.indices[nnz:] == tc.POISON_32).all() and (o.data[nnz:] == tc.POISON_32).all(), (what, "guard words behind the entries")
            if has_oov:
                assert np.array_equal(o.oov[:n_str], oov) and (o.oov[n_str:] == -7).all(), (what, "oov")


def _len_rows(rows):
    return np.array([len(r) for r in rows], np.int64)


@pytest.mark.parametrize("extra", [1, 2])
def test_term_counts_with_far_rows(gpu, scans_verified, extra):
    """n_str + 1 = (W + extra) C + 1: ticket W + extra of both row scans needs a second round (of `extra` lanes)"""
    from latok_amd import batch
    n_str = (LIM.lookback + extra) * LIM.chain_chunk
    d = tc._dict(WORDS)
    with batch.Vocab(WORDS) as vocab:
        _rows_call(gpu, n_str, lambda rows: (tc.want_vocab(rows, d), _len_rows(rows)),
                   lambda u8, boff, cap, dt: tc._call(gpu, u8, boff, vocab, cap=cap, dt=dt), True, (np.int64, np.int32))
        assert gpu.latok_debug_last_route() == tc.TERMS_ROUTE


def test_hashed_term_counts_with_far_rows(gpu, scans_verified):
    n_str = (LIM.lookback + 1) * LIM.chain_chunk
    hashed = (1 << 20, 5, True)
    _rows_call(gpu, n_str, lambda rows: (tc.want_hashed(rows, *hashed), _len_rows(rows)),
               lambda u8, boff, cap, dt: tc._call(gpu, u8, boff, hashed=hashed, cap=cap, dt=dt), False, (np.int64,))
    assert gpu.latok_debug_last_route() == tc.HASHED_ROUTE


def test_word_ngrams_with_far_rows(gpu, scans_verified):
    """(1, 2)-grams: the scan of the key rows as well"""
    from latok_amd import batch
    n_str = (LIM.lookback + 1) * LIM.chain_chunk
    rng_ = (1, 2, 0x20)
    d = tc._dict(WORDS)
    with batch.Vocab(WORDS) as vocab:
        _rows_call(gpu, n_str, lambda rows: (tc.want_vocab(ng.gram_rows(rows, *rng_), d), _len_rows(ng.gram_rows(rows, *rng_))),
                   lambda u8, boff, cap, dt: ng._call(gpu, u8, boff, rng_, vocab, cap=cap, dt=dt), True, (np.int64,))
        assert gpu.latok_debug_last_route() == ng.NGRAM_ROUTE


def test_term_counts_across_the_epoch_wrap(gpu, scans_verified):
    """every call runs three chained scans (token ranks, row starts, indptr); the multi-workgroup ones meet the wrap"""
    from latok_amd import batch
    n_str = (LIM.lookback + 1) * LIM.chain_chunk
    d = tc._dict(WORDS)
    with batch.Vocab(WORDS) as vocab:
        _set_epoch(gpu, EPOCH_MASK - 3)
        _rows_call(gpu, n_str, lambda rows: (tc.want_vocab(rows, d), _len_rows(rows)),
                   lambda u8, boff, cap, dt: tc._call(gpu, u8, boff, vocab, cap=cap, dt=dt), True, (np.int64,), repeat=4)


TOKENS = [b"a", b"ab", b"abc", b"q", b"abq", b"bc", b"ac", b"cab"]          # 1 to 3 bytes; one piece, two pieces, unknown
WP_WORDS = [b"a", b"ab", b"##c", b"bc", b"c", b"##ab", b"##b"]


def _expand_pieces(table, tp, per_string):
    """(indptr, ids, spans) of strings of per_string tokens each, single spaces between them, from the pieces of every token pattern"""
    indptr5, ids5, spans5 = table
    first = np.concatenate(([0], np.cumsum(per_string)))
    tlen = np.array([len(t) for t in TOKENS], np.int64)[tp]
    pos = np.cumsum(tlen + 1) - (tlen + 1)                                    # token starts if the batch were one string
    string_of = np.repeat(np.arange(per_string.size), per_string)
    live = per_string > 0
    base = np.zeros(per_string.size, np.int64)
    base[live] = pos[first[:-1][live]]
    start = pos - base[string_of]
    d = np.diff(indptr5)[tp]
    ends = np.concatenate(([0], np.cumsum(d)))
    src = np.repeat(indptr5[:-1][tp], d) + (np.arange(int(ends[-1])) - np.repeat(ends[:-1], d))
    return ends[first], ids5[src], spans5[src] + np.repeat(start, d)[:, None]


def test_wordpiece_with_far_tokens(gpu, scans_verified):
    """a few strings whose tokens total n_tok + 1 = (W + 1) C + 1: the scan of the pieces per token takes a second round"""
    from latok_amd import _lib, batch
    n_tok = (LIM.lookback + 1) * LIM.chain_chunk
    rng = np.random.default_rng(77)
    tp = rng.integers(0, len(TOKENS), n_tok)
    tp[:len(TOKENS)] = np.arange(len(TOKENS))
    per_string = np.array([SAMPLE, 100000, 0, 1, n_tok - SAMPLE - 100001], np.int64)
    first = np.concatenate(([0], np.cumsum(per_string)))
    blobs = [b" ".join(TOKENS[k] for k in tp[a:b].tolist()) for a, b in zip(first[:-1], first[1:])]
    u8, boff = batch.pack_utf8(blobs)
    # the patterns: every token as a string of its own, by the definition
    u5, b5 = batch.pack_utf8(TOKENS)
    indptr5, ids5, spans5, n5 = wpt.want_of(u5, b5, WP_WORDS)
    assert n5 == len(TOKENS) and set(np.diff(indptr5).tolist()) == {1, 2} and (ids5 == wpt.UNK).any()

    sample = wpt.want_of(*batch.pack_utf8(blobs[:1]), WP_WORDS)                   # the first string, SAMPLE tokens, by the definition
    got = _expand_pieces((indptr5, ids5, spans5), tp[:SAMPLE], per_string[:1])
    assert sample[3] == SAMPLE and all(np.array_equal(x, y) for x, y in zip(got, sample[:3]))
    indptr, ids, spans = _expand_pieces((indptr5, ids5, spans5), tp, per_string)
    want = (indptr, ids, spans, n_tok)
    with batch.WordPiece(WP_WORDS) as wp:
        for dt in (np.int64, np.int32):
            rc, n, got_tok, o = wpt._call(gpu, u8, boff, wp, cap=len(ids), dt=dt)
            assert rc == 0, _lib.last_error()
            assert n == len(ids) and gpu.latok_debug_last_route() == wpt.IDS_ROUTE
            wpt._compare(("far tokens", dt.__name__), o, got_tok, want, dt)
