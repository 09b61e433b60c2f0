"""SentencePiece BPE on the device (LATOK_PRETOK_SPM, latok_bpe_create_spm, include/latok_hip.h).

The result is DEFINED by tests/helpers/spbpe_ref.py, a plain restatement of the definition over bytes and one dict, which
tests/test_spbpe_host.py holds to the recorded ids of the ``sentencepiece`` and ``tokenizers`` packages.  Every batch goes through the C
ABI with poisoned guard bands round every output and is checked in full: indptr, ids, spans, the segment total, the route.  The shapes
are the smallest at which the kernels can go wrong: the sizes of a word, a tile and a workgroup of the front, of a workgroup of the cut,
of the lane form and the ceiling of max_bytes come from the library (latok_debug_pretok_limits, latok_debug_spbpe_limits)."""
import ctypes as C
import functools
import json
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from helpers import spbpe_ref as ref

pytestmark = pytest.mark.gpu

POISON_32 = np.int32(-0x5A5A5A5B)        # 0xA5A5A5A5 as int32
GUARD = 16
IDS_ROUTE, PADDED_ROUTE, SPANS_ROUTE = 30, 31, 32
UNK = -1
MARK = ref.MARK
DIR = os.path.join(GOLDEN, "spbpe")
BYTES = list(range(1000, 1256))
# ranks: a b c d <m> ab <m>a <m>ab <m><m> abab cd <m><m><m><m> e-acute
SMALL = [b"a", b"b", b"c", b"d", MARK, b"ab", MARK + b"a", MARK + b"ab", MARK + MARK, b"abab", b"cd", MARK * 4, "é".encode()]


@functools.lru_cache(maxsize=1)
def limits():
    """(segments per workgroup of the cut, the lane form's limit, the ceiling of max_bytes, bytes per word, per tile, per workgroup of the front)"""
    from latok_amd import _lib
    lib = _lib.load()
    out, pre = np.zeros(3, np.int64), np.zeros(4, np.int64)
    for fn in (lib.latok_debug_spbpe_limits, lib.latok_debug_pretok_limits):
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    assert lib.latok_debug_spbpe_limits(out.ctypes.data, 3) == 3 and lib.latok_debug_pretok_limits(pre.ctypes.data, 4) == 4
    block, lane_bytes, ceiling = map(int, out)
    word, tile, threads = int(pre[0]), int(pre[1]), int(pre[2])
    assert block % 64 == 0 and lane_bytes == 64 and ceiling == 4096 and tile % word == 0 and threads % 64 == 0
    return block, lane_bytes, ceiling, word, tile, tile * (threads // 64)


def _spm(words, ids=None, byte_ids=None, dummy=True, fuse=False, max_bytes=4096, seed=0):
    from latok_amd import batch
    return batch.BPE.sentencepiece(words, ids=ids, byte_ids=byte_ids, add_dummy_prefix=dummy, fuse_unk=fuse, max_bytes=max_bytes, seed=seed)


def want_of(blobs, words, ids=None, byte_ids=None, dummy=True, fuse=False, max_bytes=4096, unk=UNK):
    """(indptr, ids, spans[n, 2], n_segments) by the reference"""
    indptr, pids, sp = ref.encode_rows(blobs, ref.rank_dict(words), byte_ids=byte_ids, add_dummy_prefix=dummy, fuse_unk=fuse, max_bytes=max_bytes, unk=unk,
                                       ids=ids)
    return (np.array(indptr, np.int64), np.array(pids, np.int64).astype(np.int32), np.array(sp, np.int64).reshape(-1, 2),
            sum(len(ref.segments(b)) for b in blobs))


# ---- the calls, with guard bands ---------------------------------------------------------------------------------------------
class _Out:
    def __init__(self, n_str, cap, dt):
        self.indptr = np.full(n_str + 1 + GUARD, -7, dt)
        self.ids = np.full(cap + GUARD, POISON_32, np.int32)
        self.spans = np.full(2 * (cap + GUARD), -7, dt)

    def pieces_untouched(self):
        return (self.ids == POISON_32).all() and (self.spans == -7).all()


def _on_device(lib, u8, boff, arrays, call):
    """everything in device memory; the arrays are copied back"""
    from latok_amd import _lib
    sizes = [u8.nbytes + 256, boff.nbytes] + [a.nbytes for a in arrays]
    ptrs = [lib.latok_dev_alloc(s) for s in sizes]
    assert all(ptrs)
    try:
        _lib.check(lib.latok_memset_dev(ptrs[0], 0xFF, sizes[0]))
        _lib.check(lib.latok_memcpy_h2d(ptrs[0], u8.ctypes.data, u8.nbytes))
        _lib.check(lib.latok_memcpy_h2d(ptrs[1], boff.ctypes.data, boff.nbytes))
        for a, p in zip(arrays, ptrs[2:]):
            _lib.check(lib.latok_memcpy_h2d(p, a.ctypes.data, a.nbytes))
        _lib.check(lib.latok_sync())
        rc = call(ptrs[0], ptrs[1], ptrs[2:])
        for a, p in zip(arrays, ptrs[2:]):
            _lib.check(lib.latok_memcpy_d2h(a.ctypes.data, p, a.nbytes))
    finally:
        for p in ptrs:
            lib.latok_dev_free(p)
    return rc


def _call(lib, u8, boff, bpe, cap=0, dt=np.int64, unk=UNK, want_ids=True, want_spans=True, dev=False):
    """one blocking call -> (rc, n_pieces, n_segments, _Out)"""
    from latok_amd import _lib
    n_str = boff.size - 1
    total = int(boff[-1]) if n_str > 0 else 0
    o = _Out(n_str, cap, dt)
    n, n_tok = C.c_int64(-1), C.c_int64(-1)
    flags = _lib.OUT_INT32 if dt == np.int32 else 0
    if not dev:
        rc = lib.latok_bpe_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, bpe.handle, unk, o.indptr.ctypes.data,
                                                o.ids.ctypes.data if want_ids else None, o.spans.ctypes.data if want_spans else None, cap,
                                                C.byref(n), C.byref(n_tok), flags, None)
        return rc, n.value, n_tok.value, o
    rc = _on_device(lib, u8, boff, (o.indptr, o.ids, o.spans),
                    lambda d8, doff, p: lib.latok_bpe_ids_utf8_bytes_batch(d8, doff, n_str, -1, bpe.handle, unk, p[0], p[1] if want_ids else None,
                                                                           p[2] if want_spans else None, cap, C.byref(n), C.byref(n_tok),
                                                                           flags | _lib.DEVICE_PTRS, None))
    return rc, n.value, n_tok.value, o


def _compare(what, o, n_tok_got, want, dt, has_spans=True):
    indptr, ids, spans, n_tok = want
    n_str, n = len(indptr) - 1, len(ids)
    assert n_tok_got == n_tok, (what, "segment total", n_tok_got, n_tok)
    assert o.indptr.dtype == dt and np.array_equal(o.indptr[:n_str + 1], indptr), (what, "indptr", o.indptr[:n_str + 1].tolist()[:40], indptr.tolist()[:40])
    assert (o.indptr[n_str + 1:] == -7).all(), (what, "guard words behind indptr")
    if not np.array_equal(o.ids[:n], ids):
        k = int(np.nonzero(o.ids[:n] != ids)[0][0])
        s = int(np.searchsorted(indptr, k, "right")) - 1
        raise AssertionError((what, "piece", k, "of", n, "row", s, "got", int(o.ids[k]), "want", int(ids[k]), "wrong:", int((o.ids[:n] != ids).sum())))
    assert (o.ids[n:] == POISON_32).all(), (what, "guard words behind the ids")
    if has_spans:
        got = o.spans[:2 * n].reshape(-1, 2)
        if not np.array_equal(got, spans):
            k = int(np.nonzero((got != spans).any(axis=1))[0][0])
            raise AssertionError((what, "span of piece", k, "got", got[k].tolist(), "want", spans[k].tolist()))
        assert (o.spans[2 * n:] == -7).all(), (what, "guard words behind the spans")
    else:
        assert (o.spans == -7).all()


# width of indptr / spans x host / device pointers x with / without spans
FORMS = ((np.int64, False, True), (np.int32, True, True), (np.int32, False, True), (np.int64, True, True), (np.int64, False, False), (np.int32, True, False))


def check(lib, blobs, words, what="", forms=FORMS[:2], unk=UNK, seed=0, **kw):
    """the whole definition for one batch; returns want = (indptr, ids, spans, n_segments)"""
    from latok_amd import _lib, batch
    u8, boff = batch.pack_utf8(blobs)
    if u8.size == 0:
        u8 = np.zeros(1, np.uint8)
    want = want_of(blobs, words, unk=unk, **kw)
    need = len(want[1])
    with _spm(words, seed=seed, **kw) as bpe:
        for dt, dev, with_spans in forms:
            rc, n, n_tok, o = _call(lib, u8, boff, bpe, cap=need, dt=dt, unk=unk, dev=dev, want_spans=with_spans)
            assert rc == 0, (what, _lib.last_error())
            assert n == need, (what, n, need)
            assert lib.latok_debug_last_route() == IDS_ROUTE or int(boff[-1]) == 0
            _compare((what, dt.__name__, "device" if dev else "host"), o, n_tok, want, dt, has_spans=with_spans)
    return want


def _rows(want):
    return [list(zip(want[1][a:b].tolist(), *want[2][a:b].T.tolist())) for a, b in zip(want[0][:-1], want[0][1:])]


# ---- 1. the segments ---------------------------------------------------------------------------------------------------------
def _segments_call(lib, blobs, dt, dev):
    from latok_amd import _lib, batch
    u8, boff = batch.pack_utf8(blobs)
    if u8.size == 0:
        u8 = np.zeros(1, np.uint8)
    n_str, total = len(blobs), int(boff[-1])
    want = [ref.segments(b) for b in blobs]
    n_want = sum(map(len, want))
    counts = np.full(n_str + GUARD, -7, dt)
    spans = np.full(2 * (n_want + GUARD), -7, dt)
    n = C.c_int64(-1)
    flags = _lib.OUT_INT32 if dt == np.int32 else 0
    if dev:
        rc = _on_device(lib, u8, boff, (counts, spans),
                        lambda d8, doff, p: lib.latok_pretokens_utf8_bytes_batch(d8, doff, n_str, -1, _lib.PRETOK_SPM, p[0], p[1], n_want, C.byref(n),
                                                                                 flags | _lib.DEVICE_PTRS, None))
    else:
        rc = lib.latok_pretokens_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, _lib.PRETOK_SPM, counts.ctypes.data, spans.ctypes.data,
                                                  n_want, C.byref(n), flags, None)
    assert rc == 0, _lib.last_error()
    assert n.value == n_want and (lib.latok_debug_last_route() == SPANS_ROUTE or total == 0)
    assert counts[:n_str].tolist() == [len(w) for w in want] and (counts[n_str:] == -7).all()
    got = spans[:2 * n_want].reshape(-1, 2).tolist()
    flat = [list(s) for w in want for s in w]
    if got != flat:
        k = next(i for i, (a, b) in enumerate(zip(got, flat)) if a != b)
        raise AssertionError(("segment", k, "got", got[k], "want", flat[k], dt.__name__, dev))
    assert (spans[2 * n_want:] == -7).all()


SEGMENT_BLOBS = ([b" " * k + b"ab" for k in range(6)] + [(b" " + MARK) * k + b"x" for k in range(4)] + [MARK * k + b" q" for k in range(4)] +
                 [b"in" + MARK + b"side", b"in" + MARK + MARK + b" side", b"trail  ", b"trail" + MARK, b"   ", b" ", MARK, b"", b"", b"a b", b"end ", b"next", b"x ",
                  b" y", MARK + b"\x80 a", b"a" + MARK + b"\xbf", b"cut \xe2\x96", b"\xe2\x96", b"\x81 z", b"a\tb\nc d", b"\x80\x80", b" \x80 ",
                  "日本 語 テ".encode(), b"a \xe2\x96\x81\xe2\x96 b", b"\xe2 \x96\x81"])


def test_the_segments(gpu):
    for dt, dev in ((np.int64, False), (np.int32, True), (np.int32, False), (np.int64, True)):
        _segments_call(gpu, SEGMENT_BLOBS, dt, dev)
    _segments_call(gpu, [b"", b""], np.int64, False)


def test_segment_starts_at_every_offset_and_across_tiles_and_workgroups(gpu):
    """segment starts at every offset mod 4 and at 62 .. 65 mod 64; a segment (and a three-byte marker) straddling a word, a tile and a
    workgroup edge of the front"""
    _, _, _, word, tile, group = limits()
    blobs, at = [], 0
    for edge in (word, 2 * word, tile, group, group + tile):
        for back in range(0, 5):                      # a marker that begins `back` bytes in front of the edge
            pad = edge - back - at - 1
            if pad < 2:
                continue
            blobs.append(b"w" * (pad - 1) + b" " + b"z" + MARK + b"ab " + MARK + b" cd")
            at += len(blobs[-1])
    for off in (62, 63, 64, 65, 66, 67):
        blobs.append(b"q" * (off - at % 64 + 64) + b" x")
        at += len(blobs[-1])
    long_seg = b" " + b"abcd" * (tile // 4 + 5)      # a segment longer than a tile
    blobs += [long_seg, b"k" * 3 + MARK * 40 + b"r", b" " * 130]
    assert sum(map(len, blobs)) > group + tile
    _segments_call(gpu, blobs, np.int64, False)
    _segments_call(gpu, blobs, np.int32, True)
    from latok_amd import batch
    assert batch.pretokenize_utf8_batch(blobs[:8], "spm") == [[b[a:e] for a, e in ref.segments(b)] for b in blobs[:8]]


def test_pretokenize_batch(gpu):
    from latok_amd import batch
    texts = ["hello  world", " a", "", "x▁y z", "tab\tbed new\nline", "日本 語", "   "]
    want = [[t.encode()[a:e].decode() for a, e in ref.segments(t.encode())] for t in texts]
    assert batch.pretokenize_batch(texts, "spm") == want
    assert want[0] == ["hello", "  world"] and want[3] == ["x", "▁y", " z"] and want[2] == []
    assert all("".join(r) == t for r, t in zip(want, texts))


# ---- 2. the cut: virtual lengths -----------------------------------------------------------------------------------------------
def _of_len(n):
    return b"ab" * (n // 2) + b"c" * (n % 2)


def test_virtual_lengths_round_the_lane_limit(gpu):
    """1 .. 4 and 62 .. 66 reached by real bytes and by marker expansion (58 real bytes behind 2 spaces plus the dummy = 67 ...)"""
    blobs = []
    for L in list(range(1, 5)) + list(range(60, 68)):
        blobs += [_of_len(L), b"k " + _of_len(max(L - 3, 1)), b"k  " + _of_len(max(L - 6, 1)), b" " + _of_len(max(L - 6, 1))]
    blobs += [b"  " + _of_len(58), b"  " + _of_len(57), b"  " + _of_len(55), MARK * 3 + _of_len(52)]
    for dummy in (False, True):
        want = check(gpu, blobs, SMALL, what=("lengths", dummy), forms=FORMS, dummy=dummy, byte_ids=BYTES)
        assert (want[1] < 1000).sum() > 100
    check(gpu, blobs, SMALL, what="lengths, unk", dummy=True, fuse=True)


def test_max_bytes_edges(gpu):
    blobs = []
    for L in (7, 8, 9):
        blobs += [_of_len(L), b"z " + _of_len(L - 3), b"z" + b" " * (L // 3) + b"a" * (L % 3), b" " * ((L - 3) // 3) + b"a" * ((L - 3) % 3)]
    for dummy, by in ((False, None), (True, BYTES)):
        want = check(gpu, blobs, SMALL, what=("max_bytes", 8, dummy), max_bytes=8, dummy=dummy, byte_ids=by, fuse=by is None)
        assert (want[1] == UNK).any()
    # the ceiling: real bytes alone without the dummy; a lead run of markers in front with it (the reference rescans every part in every
    # round: a few hundred merges per segment keep it quick)
    plain = [b"ab" * 100 + b"c" * (L - 200) for L in (4095, 4096, 4097)]
    want = check(gpu, plain, SMALL, what=("max_bytes", 4096, "bytes"), max_bytes=4096, dummy=False, fuse=True)
    assert np.diff(want[0]).tolist()[2] == 1 and want[1][-1] == UNK and np.diff(want[0]).tolist()[0] > 1000
    led = [b" " * 300 + b"d" * (L - 903) for L in (4095, 4096, 4097)]
    want = check(gpu, led, SMALL, what=("max_bytes", 4096, "lead run"), max_bytes=4096, dummy=True, byte_ids=BYTES)
    assert np.diff(want[0]).tolist()[2] == 1 and want[1][-1] == UNK and want[2][-1].tolist() == [0, len(led[2])]
    with _spm(SMALL, max_bytes=9) as bpe:
        assert bpe.info()["max_bytes"] == 9 and bpe.spm_info() == dict(byte_fallback=0, add_dummy_prefix=1, fuse_unk=0)


def test_a_wave_form_segment_whose_lead_run_alone_passes_64_bytes(gpu):
    blobs = [b"x" + b" " * 22 + b"ab", b"x" + b" " * 30 + b"abab", b"x" + (b" " + MARK) * 15 + b"cd", b"x" + MARK * 70 + b"a", b" " * 100, b"x" + b" " * 400 + _of_len(300),
             b"y" + (MARK + b"  ") * 40 + b"abab"]
    want = check(gpu, blobs, SMALL, what="long lead", forms=FORMS, byte_ids=BYTES)
    assert _rows(want)[0][:3] == [(4, 0, 0), (1000 + ord("x"), 0, 1), (11, 1, 5)]         # the dummy alone: an empty span
    assert _rows(want)[4] == [(11, 0, 3)] + [(11, 3 + 4 * k, 7 + 4 * k) for k in range(24)] + [(4, 99, 100)]   # 101 markers: 25 fours and one
    check(gpu, blobs, SMALL, what="long lead, no dummy, fused", dummy=False, fuse=True)


# ---- 3. no shortcut, ranks -------------------------------------------------------------------------------------------------------
def test_no_whole_segment_shortcut(gpu):
    """abc without ab and bc gives a b c; the same text through a latok_bpe_create object gives one piece"""
    from latok_amd import batch
    words = [b"a", b"b", b"c", b"abc"]
    want = check(gpu, [b"abc", b"abc abc"], words, what="no shortcut", dummy=False, forms=FORMS)
    assert _rows(want)[0] == [(0, 0, 1), (1, 1, 2), (2, 2, 3)]
    with batch.BPE(words) as plain:
        indptr, ids, _ = batch.bpe_ids_utf8_batch([b"abc"], plain)
        assert ids.tolist() == [3] and plain.pretokenizer_of_object() == "latok"
    with _spm(words, dummy=False) as bpe:
        assert bpe.pretokenizer_of_object() == "spm"
        assert batch.bpe_ids_utf8_batch([b"abc"], bpe)[1].tolist() == [0, 1, 2]


def test_ranks_leftmost_among_equals_and_rank_beats_position(gpu):
    words = [b"a", b"b", b"ab", b"ab", b"ba", b"aba"]
    want = check(gpu, [b"ababab", b"bababa", b"aabab", b"ab" * 40], words, what="equal ranks", dummy=False, forms=FORMS)
    assert [(a, e) for _, a, e in _rows(want)[0]] == [(0, 2), (2, 4), (4, 6)]
    words2 = [b"a", b"b", b"c", b"bc", b"ab"]
    want = check(gpu, [b"abc", b"abcabc", b"ababc", b"abc" * 30], words2, what="rank beats position", dummy=False)
    assert [(a, e) for _, a, e in _rows(want)[0]] == [(0, 1), (1, 3)]


# ---- 4. byte fallback --------------------------------------------------------------------------------------------------------------
def test_byte_fallback(gpu):
    blobs = [b"a~b", "aßb".encode(), "a€b".encode(), "a😀b".encode(), b"\x80a", b"a\xbf\xbf", b"ab\xe2\x96", b"\xf0\x9f", "日本語".encode() * 30, b"~" * 70]
    want = check(gpu, blobs, SMALL, what="byte fallback", forms=FORMS, byte_ids=BYTES, dummy=False)
    rows = _rows(want)
    assert rows[0] == [(0, 0, 1), (1000 + 0x7E, 1, 2), (1, 2, 3)]
    assert rows[2] == [(0, 0, 1), (1000 + 0xE2, 1, 4), (1000 + 0x82, 1, 4), (1000 + 0xAC, 1, 4), (1, 4, 5)]
    assert [p[0] for p in rows[3]] == [0, 1240, 1159, 1152, 1128, 1]
    # the marker absent from the vocabulary: three byte pieces with one shared span; for the dummy an empty span
    words = [b"a", b"b", b"ab"]
    want = check(gpu, [b"a b", b" ", b"ab", b""], words, what="marker absent", forms=FORMS, byte_ids=BYTES, dummy=True)
    rows = _rows(want)
    m3 = [1000 + 0xE2, 1000 + 0x96, 1000 + 0x81]
    assert rows[0] == [(i, 0, 0) for i in m3] + [(0, 0, 1)] + [(i, 1, 2) for i in m3] + [(1, 2, 3)]
    assert rows[1] == [(i, 0, 0) for i in m3] + [(i, 0, 1) for i in m3] and rows[2] == [(i, 0, 0) for i in m3] + [(2, 0, 2)] and rows[3] == []
    assert len(want[1]) > sum(map(len, [b"a b", b" ", b"ab"]))          # more pieces than bytes


def test_capacity_with_more_pieces_than_bytes(gpu):
    """the size query, a capacity too small by one, the exact one -- where byte fallback makes more pieces than the batch has bytes"""
    from latok_amd import _lib, batch
    words = [b"a", b"b", b"ab"]
    blobs = [b"a b", b" ", b"ab  ", b"", b" " * 70]
    u8, boff = batch.pack_utf8(blobs)
    want = want_of(blobs, words, byte_ids=BYTES)
    need = len(want[1])
    assert need > int(boff[-1]) * 2
    with _spm(words, byte_ids=BYTES) as bpe:
        for dev in (False, True):
            rc, n, n_tok, o = _call(gpu, u8, boff, bpe, cap=0, want_ids=False, want_spans=False, dev=dev)
            assert rc == _lib.ERR_INVALID and n == need and n_tok == want[3] and o.pieces_untouched() and np.array_equal(o.indptr[:len(blobs) + 1], want[0])
            rc, n, n_tok, o = _call(gpu, u8, boff, bpe, cap=need - 1, dev=dev)
            assert rc == _lib.ERR_INVALID and "capacity" in _lib.last_error() and n == need and o.pieces_untouched()
            rc, n, n_tok, o = _call(gpu, u8, boff, bpe, cap=need, dev=dev)
            assert rc == 0
            _compare(("exact", dev), o, n_tok, want, np.int64)
            rc, n, n_tok, o = _call(gpu, u8, boff, bpe, cap=need + 5, dt=np.int32, dev=dev)
            assert rc == 0
            _compare(("roomy", dev), o, n_tok, want, np.int32)


# ---- 5. without byte ids; the dummy prefix -----------------------------------------------------------------------------------------
def test_unknown_pieces_fused_and_not(gpu):
    blobs = [b"a~~b", b"~~", b"a~ ~b", b"~a~", "a日本b €€".encode(), b"ab~", b"~" * 70 + b"ab" + b"~" * 70, b"a" + b"~" * 64, b"~" * 63 + b"a~"]
    plain = check(gpu, blobs, SMALL, what="unk", forms=FORMS, fuse=False, dummy=False)
    fused = check(gpu, blobs, SMALL, what="fused unk", forms=FORMS, fuse=True, dummy=False)
    assert _rows(plain)[0] == [(0, 0, 1), (UNK, 1, 2), (UNK, 2, 3), (1, 3, 4)] and _rows(fused)[0] == [(0, 0, 1), (UNK, 1, 3), (1, 3, 4)]
    assert _rows(fused)[1] == [(UNK, 0, 2)] and _rows(fused)[2] == [(0, 0, 1), (UNK, 1, 2), (4, 2, 3), (UNK, 3, 4), (1, 4, 5)]   # a run ends at a segment edge
    assert _rows(fused)[6] == [(UNK, 0, 70), (5, 70, 72), (UNK, 72, 142)]
    check(gpu, blobs, SMALL, what="fused unk, dummy", fuse=True, dummy=True, unk=7)


def test_the_dummy_prefix(gpu):
    blobs = [b"ab", b" ab", b"  ab", b"a", b" ", b"", MARK + b"ab", b"ab ab"]
    on = check(gpu, blobs, SMALL, what="dummy on", forms=FORMS, dummy=True, byte_ids=BYTES)
    off = check(gpu, blobs, SMALL, what="dummy off", forms=FORMS, dummy=False, byte_ids=BYTES)
    assert _rows(on)[0] == [(7, 0, 2)] and _rows(off)[0] == [(5, 0, 2)]
    assert _rows(on)[1] == [(4, 0, 0), (7, 0, 3)] and _rows(off)[1] == [(7, 0, 3)]          # ab, then <m>ab, outrank <m><m>: the dummy stays alone
    assert _rows(on)[2] == [(8, 0, 1), (7, 1, 4)] and _rows(off)[2] == [(4, 0, 1), (7, 1, 4)]
    assert _rows(on)[4] == [(8, 0, 1)] and _rows(off)[4] == [(4, 0, 1)] and _rows(on)[5] == [] and _rows(on)[6] == [(4, 0, 0), (7, 0, 5)]
    assert _rows(on)[7] == [(7, 0, 2), (7, 2, 5)] and _rows(off)[7] == [(5, 0, 2), (7, 2, 5)]   # only a string's first segment has it


# ---- 6. the padded form -------------------------------------------------------------------------------------------------------------
def test_the_padded_form_truncates_inside_a_byte_fallback_character(gpu):
    from latok_amd import _lib, batch
    blobs = ["a€b".encode(), b"", b"ab ab ab", "😀".encode(), b" "]
    u8, boff = batch.pack_utf8(blobs)
    want = want_of(blobs, SMALL, byte_ids=BYTES, dummy=False)
    assert want[1][:5].tolist() == [0, 1226, 1130, 1172, 1]
    with _spm(SMALL, byte_ids=BYTES, dummy=False) as bpe:
        for max_length, special in ((3, False), (5, True), (2, False), (16, True)):
            block = np.full(len(blobs) * max_length + GUARD, POISON_32, np.int32)
            lengths = np.full(len(blobs) + GUARD, POISON_32, np.int32)
            n = C.c_int64(-1)
            rc = gpu.latok_bpe_padded_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, len(blobs), int(boff[-1]), bpe.handle, UNK, max_length, int(special),
                                                       101, 102, -9, block.ctypes.data, lengths.ctypes.data, C.byref(n), 0, None)
            assert rc == 0 and n.value == len(want[1]), _lib.last_error()
            assert gpu.latok_debug_last_route() == PADDED_ROUTE
            for s in range(len(blobs)):
                body = want[1][want[0][s]:want[0][s + 1]].tolist()[:max_length - 2 * special]
                row = ([101] if special else []) + body + ([102] if special else [])
                assert block[s * max_length:(s + 1) * max_length].tolist() == row + [-9] * (max_length - len(row)), (s, max_length, special)
                assert lengths[s] == len(row)
            assert (block[len(blobs) * max_length:] == POISON_32).all() and (lengths[len(blobs):] == POISON_32).all()
        ids, mask = batch.bpe_encode_utf8_batch(blobs, bpe, 3)
        assert ids[0].tolist() == [0, 1226, 1130] and mask[1].sum() == 0       # cut between the second and the third byte of the euro sign


# ---- 7. parity with the packages' recorded ids ------------------------------------------------------------------------------------
@pytest.mark.parametrize("loader", ["model", "tokenizer_json"])
def test_the_recorded_sentencepiece_ids(gpu, loader):
    from latok_amd import batch
    with open(os.path.join(DIR, "spbpe_cases.json"), encoding="utf-8") as f:
        cases = json.load(f)["cases"]
    assert len(cases) >= 200
    make = ((lambda: batch.BPE.from_sentencepiece_model(os.path.join(DIR, "m.model"))) if loader == "model" else
            (lambda: batch.BPE.from_spm_tokenizer_json(os.path.join(DIR, "tokenizer.json"))))
    with make() as bpe:
        assert bpe.spm_info() == dict(byte_fallback=1, add_dummy_prefix=1, fuse_unk=1) and bpe.unk_id == 0 and bpe.pretokenizer_of_object() == "spm"
        indptr, ids, spans = batch.bpe_ids_utf8_batch([c["text"].encode() for c in cases], bpe, unk_id=bpe.unk_id)
        for k, c in enumerate(cases):
            assert ids[indptr[k]:indptr[k + 1]].tolist() == c["sp_ids"], c["text"]
        assert gpu.latok_debug_last_route() == IDS_ROUTE
        got = batch.bpe_ids_batch([c["text"] for c in cases[:20]], bpe)
        assert got[1].tolist() == [i for c in cases[:20] for i in c["sp_ids"]]


# ---- 8. more than one workgroup, random text, malformed bytes ------------------------------------------------------------------------
def test_random_text_over_several_workgroups(gpu):
    from latok_amd.batch import BPE
    block = limits()[0]
    words, ids, byte_ids, _, _ = BPE.sentencepiece_word_list(os.path.join(DIR, "m.model"))
    rng = random.Random(9)
    units = [b"the", b"quick", b"token", b"model", b"hello", b"ab", b"x", "日本語".encode(), "naïve".encode(), "😀".encode(), b"\x80", b"\xe2\x96", MARK, b"\t", b"\n"]
    blobs = []
    for _ in range(300):
        blobs.append(b"".join(rng.choice(units) + rng.choice([b" ", b" ", b"  ", b"", b"   "]) for _ in range(rng.randint(0, 14))))
    blobs += [b"token" * 30, ("日本語".encode() * 40) + b" x", b" " * 200 + b"the"]
    want = check(gpu, blobs, words, what="random", forms=FORMS[:2], ids=ids, byte_ids=byte_ids)
    assert want[3] > 3 * block
    check(gpu, blobs[:120], words, what="random, no bytes", forms=FORMS[2:4], ids=ids, fuse=True, dummy=False, unk=0, seed=12345)


# ---- 9. one shared object, two contexts at once ------------------------------------------------------------------------------------
def test_one_object_used_from_two_contexts_concurrently(gpu):
    from latok_amd import batch
    from test_gpu_shared_objects import _run_workers
    rng = random.Random(21)
    batches = []
    for n in (40, 400):
        blobs = [b" ".join(_of_len(rng.randint(1, 20)) for _ in range(rng.randint(0, 9))) + rng.choice([b"", b" ", "€".encode()]) for _ in range(n)]
        batches.append((blobs, want_of(blobs, SMALL, byte_ids=BYTES)))
    with _spm(SMALL, byte_ids=BYTES) as bpe:
        def job(k, gate):
            for r in range(4):
                blobs, want = batches[(k + r) % 2]
                indptr, ids, spans = batch.bpe_ids_utf8_batch(blobs, bpe)
                assert np.array_equal(indptr, want[0]) and np.array_equal(ids, want[1]) and np.array_equal(spans, want[2]), (k, r)
                gate.wait()

        _run_workers([job, job])


# ---- 10. refusals on the device's side, the example ---------------------------------------------------------------------------------
def test_spm_info_refuses_other_objects(gpu):
    from latok_amd import _lib, batch
    with batch.BPE([b"a", b"b"]) as plain:
        with pytest.raises(Exception):
            plain.spm_info()
        assert "latok_bpe_create_spm" in _lib.last_error()
    with pytest.raises(Exception):
        _spm([b"a", b"a" + MARK])
    assert "word 1 " in _lib.last_error()


def test_c_example(gpu, tmp_path):
    exe = str(tmp_path / "spbpe_utf8")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "spbpe_utf8.c"),
                           "-L" + os.path.join(ROOT, "latok_amd"), "-llatok_hip", "-Wl,-rpath," + os.path.join(ROOT, "latok_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[:4] == ["  row 0: [0,3) [3,10)", "  row 1:", "  row 2: [0,3)", "  row 3: [0,3) [3,6)"]
    m = MARK
    words = [m + b"l", b"lo", m + b"lo", m + b"low", m + m, b"l", b"o", b"w", m, b"e", b"r", b"er"]
    texts = [b"low  lower", b"", b"   ", b"low \xc3\xa9"]
    want = want_of(texts, words, ids=[300 + i for i in range(12)], byte_ids=[3 + b for b in range(256)], unk=0)
    assert lines[4] == "%d segments, %d pieces" % (want[3], len(want[1]))
    for s, row in enumerate(_rows(want)):
        assert lines[5 + s] == "  row %d:" % s + "".join(" %d[%d,%d)" % p for p in row)
