"""Decoding on the device (latok_detok_csr / latok_detok_padded, batch.Detokenizer) against tests/helpers/detok_ref.py: both modes, CSR
and padded forms, host and device pointers, int32 and int64 indptr; piece counts around one and two workgroups, a batch of more
workgroups than one workgroup of the chained scan holds, empty rows and rows across workgroup edges; the LDS window (1-byte words,
words of window - 1 / window / window + 1 bytes and of several windows, output starts at every byte phase mod 16, sentinels around
every output); the capacity protocol to the letter; unknown ids; round trips through the BPE and WordPiece encoders, CSR and padded;
malformed rows refused with the buffers untouched; two contexts on one object at once, and destroy behind the last call.  The sizes
come from latok_debug_detok_limits.  Nothing here provokes a fault: malformed rows are refused by the validation kernels."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

from conftest import ALPHABETS, random_strings
from helpers import bpe_ref
from helpers import detok_ref as ref

pytestmark = pytest.mark.gpu

SENT = 0x5A
DEVICE_PTRS, OUT_INT32 = 1, 2        # LATOK_DEVICE_PTRS, LATOK_OUT_INT32
WP_WORDS = [b"[PAD]", b"[CLS]", b"[SEP]", b"un", b"##aff", b"##able", b"##", b"a b", b"", b"##\xc3\xa9t\xc3\xa9", b"x", b"##y", b"#", b"###", b"the",
            b"##s", b"q"]


def _limits():
    from latok_amd import _lib
    fn = _lib.load().latok_debug_detok_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(5, np.int64)
    assert fn(out.ctypes.data, 5) == 5
    return [int(x) for x in out]


def test_the_flag_values_are_the_headers():
    from latok_amd import _lib
    assert (_lib.DEVICE_PTRS, _lib.OUT_INT32) == (DEVICE_PTRS, OUT_INT32)


class _Dev:
    """device copies of host arrays, freed together"""

    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def alloc(self, nbytes):
        p = self.lib.latok_dev_alloc(nbytes + 64)
        assert p
        self.ptrs.append(p)
        return p

    def put(self, a):
        from latok_amd import _lib
        p = self.alloc(a.nbytes)
        if a.nbytes:
            _lib.check(self.lib.latok_memcpy_h2d(p, a.ctypes.data, a.nbytes))
        return p

    def get(self, p, a):
        from latok_amd import _lib
        if a.nbytes:
            _lib.check(self.lib.latok_memcpy_d2h(a.ctypes.data, p, a.nbytes))
        return a

    def close(self):
        for p in self.ptrs:
            self.lib.latok_dev_free(p)


def _call(lib, detok, rows=None, block=None, lengths=None, skip=(), dev=False, i32=False, cap=None, phase=0, query=False, indptr=None, ids=None):
    """One call with sentinels around every output.  rows: a CSR from lists (or indptr / ids given raw); block: the padded form.
    cap: None = room for anything (the reference's need is not used), else the capacity passed.  Returns (rc, n, unknown, out bytes
    [0 .. cap), out_off) after checking that nothing around the outputs moved."""
    from latok_amd import _lib
    padded = block is not None
    if padded:
        block = np.ascontiguousarray(block, np.int32)
        n_rows, max_length = block.shape
        first = block.reshape(-1)
        second = None if lengths is None else np.ascontiguousarray(lengths, np.int32)
    else:
        if indptr is None:
            indptr = np.zeros(len(rows) + 1, np.int64)
            np.cumsum([len(r) for r in rows], out=indptr[1:])
            ids = np.array([i for r in rows for i in r], np.int32)
        n_rows = indptr.size - 1
        first = np.ascontiguousarray(indptr, np.int32 if i32 else np.int64)
        second = np.ascontiguousarray(ids, np.int32)
    skip_a = np.array(list(skip) + [0], np.int32)
    room = 1 << 16 if cap is None else cap
    pad = 32
    out = np.full(pad + phase + room + pad, SENT, np.uint8)
    off = np.full(n_rows + 1 + 4, -7, np.int64)
    n, unk = C.c_int64(-1), C.c_int64(-1)
    flags = (DEVICE_PTRS if dev else 0) | (OUT_INT32 if i32 and not padded else 0)
    d = _Dev(lib)
    try:
        if dev:
            p_first, p_second = d.put(first), (d.put(second) if second is not None else None)
            p_out, p_off = d.put(out), d.put(off)
            a_out, a_off = p_out + pad + phase, p_off
        else:
            p_first, p_second = first.ctypes.data, (second.ctypes.data if second is not None else None)
            a_out, a_off = out.ctypes.data + pad + phase, off.ctypes.data
        if query:
            a_out, room = None, 0
        if padded:
            rc = lib.latok_detok_padded(detok.handle, p_first, p_second, n_rows, max_length, skip_a.ctypes.data, len(skip), a_out, room, a_off, C.byref(n),
                                        C.byref(unk), flags, None)
        else:
            rc = lib.latok_detok_csr(detok.handle, p_first, p_second, n_rows, second.size, skip_a.ctypes.data, len(skip), a_out, room, a_off, C.byref(n),
                                     C.byref(unk), flags, None)
        if dev:
            d.get(p_out, out)
            d.get(p_off, off)
    finally:
        d.close()
    assert (out[:pad + phase] == SENT).all() and (off[n_rows + 1:] == -7).all(), "a byte in front of the output or behind out_off moved"
    written = n.value if rc == _lib.OK and not query else 0
    assert (out[pad + phase + written:] == SENT).all(), "a byte behind the output moved"
    return rc, n.value, unk.value, out[pad + phase:pad + phase + written].tobytes(), off[:n_rows + 1].copy()


def _check(lib, detok, d, rows, mode, prefix=b"##", sep=b" ", skip=(), **kw):
    from latok_amd import _lib
    want, unknown = ref.decode(rows, d, mode, prefix, sep, skip)
    rc, n, unk, out, off = _call(lib, detok, rows=rows, skip=skip, **kw)
    assert rc == _lib.OK, _lib.last_error()
    want_off = np.cumsum([0] + [len(w) for w in want])
    assert n == want_off[-1] and unk == unknown and np.array_equal(off, want_off), (n, unk, unknown)
    assert out == b"".join(want)


def _rows_of(rng, n_pieces, pool, shape):
    """n_pieces ids cut into rows: 'short' rows of 0 .. 12, 'long' = a few rows that span workgroups, 'empties' = runs of empty rows"""
    ids = [rng.choice(pool) for _ in range(n_pieces)]
    cuts = {0, n_pieces}
    if shape == "short":
        k = 0
        while k < n_pieces:
            k += rng.randint(0, 12)
            cuts.add(min(k, n_pieces))
    elif shape == "long":
        cuts.update(rng.randrange(n_pieces + 1) for _ in range(3))
    cuts = sorted(cuts)
    rows = [ids[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    if shape != "long":
        at = rng.randrange(len(rows) + 1)
        rows[at:at] = [[] for _ in range(300 if shape == "empties" else 3)]
        rows = [[]] + rows + [[], []]
    return rows


@pytest.fixture(scope="module")
def objects(gpu):
    from latok_amd import batch
    made = dict(
        wp=batch.Detokenizer(WP_WORDS, mode="wordpiece", prefix=b"##", sep=b" "),
        concat=batch.Detokenizer(WP_WORDS),
        sparse=batch.Detokenizer(WP_WORDS, ids=[(i - 8) * 1000003 for i in range(len(WP_WORDS))], mode="wordpiece", prefix=b"##", sep=b"_"))
    yield made
    for o in made.values():
        o.close()


def test_info_says_which_form_the_map_took(objects):
    spread = _limits()[2]
    info = objects["wp"].info()
    assert info["dense"] == 1 and info["mode"] == 1 and info["n_words"] == info["n_ids"] == len(WP_WORDS) == len(objects["wp"])
    assert info["max_len"] == max(map(len, WP_WORDS)) and info["blob_bytes"] == sum((len(w) + 3) // 4 * 4 for w in WP_WORDS)
    assert objects["sparse"].info()["dense"] == 0 and objects["concat"].info()["mode"] == 0
    assert not ref.is_dense(WP_WORDS, [(i - 8) * 1000003 for i in range(len(WP_WORDS))], spread)


@pytest.mark.parametrize("which", ["wp", "concat", "sparse"])
def test_piece_counts_around_one_and_two_workgroups(gpu, objects, which):
    block = _limits()[0]
    detok = objects[which]
    ids_of = [(i - 8) * 1000003 for i in range(len(WP_WORDS))] if which == "sparse" else list(range(len(WP_WORDS)))
    d = ref.id_map(WP_WORDS, ids_of)
    mode, sep = (ref.CONCAT, b"") if which == "concat" else (ref.WORDPIECE, b"_" if which == "sparse" else b" ")
    pool = ids_of + [ids_of[0]] * 4 + [12345, -1]
    rng = random.Random(7)
    k = 0
    for n_pieces in (1, block - 1, block, block + 1, 2 * block - 1, 2 * block, 2 * block + 1):
        for shape in ("short", "long", "empties"):
            rows = _rows_of(rng, n_pieces, pool, shape)
            for skip in ((), (ids_of[0], ids_of[1], ids_of[2])):
                _check(gpu, detok, d, rows, mode, sep=sep, skip=skip, dev=bool(k & 1), i32=bool(k & 2))
                k += 1
    for dev in (False, True):
        for i32 in (False, True):
            _check(gpu, detok, d, [[]] * 5, mode, sep=sep, dev=dev, i32=i32)
            _check(gpu, detok, d, [[ids_of[3]], [], [ids_of[4], ids_of[5]]], mode, sep=sep, dev=dev, i32=i32, skip=tuple(range(100, 116)))


def test_a_batch_of_more_workgroups_than_one_scan_workgroup_holds(gpu):
    """1-byte words, so the reference is numpy: out = table[kept ids], out_off = kept pieces in front of every row"""
    from latok_amd import _lib, batch
    block, _, _, chunk, _ = _limits()
    n = block * chunk + block + 3
    rng = np.random.default_rng(3)
    table = np.arange(33, 33 + 90, dtype=np.uint8)
    with batch.Detokenizer([bytes([b]) for b in table]) as detok:
        ids = rng.integers(0, 92, n).astype(np.int32)           # 90 and 91 are unknown, 5 is skipped
        kept = (ids < 90) & (ids != 5)
        cuts = np.unique(np.concatenate([[0, n], rng.integers(0, n + 1, 5000)]))
        indptr = np.concatenate([[0, 0], cuts[1:-1], [n, n, n]]).astype(np.int64)
        rank = np.concatenate([[0], np.cumsum(kept)])
        want = table[ids[kept]].tobytes()
        for dev, i32 in ((True, False), (False, True)):
            rc, got_n, unk, out, off = _call(gpu, detok, indptr=indptr, ids=ids, skip=(5,), dev=dev, i32=i32, cap=n)
            assert rc == _lib.OK and got_n == len(want) and unk == int((ids >= 90).sum())
            assert np.array_equal(off, rank[indptr]) and out == want


def test_the_padded_form_lengths_and_pad(gpu, objects):
    from latok_amd import _lib
    block_sz = _limits()[0]
    d = ref.id_map(WP_WORDS)
    rng = random.Random(11)
    for n_rows, L in ((1, 1), (3, 7), (5, block_sz + 1), (block_sz + 3, 5), (2, 2 * block_sz)):
        block = np.array([[rng.choice(range(len(WP_WORDS) + 1)) for _ in range(L)] for _ in range(n_rows)], np.int32)
        lengths = np.array([rng.choice((0, L, rng.randint(0, L))) for _ in range(n_rows)], np.int32)
        lengths[0], lengths[-1] = L, 0
        for which, mode in (("wp", ref.WORDPIECE), ("concat", ref.CONCAT)):
            for lens, skip in ((lengths, (1, 2)), (None, (0,)), (None, tuple(range(16)))):
                want, unknown = ref.decode(ref.padded_rows(block.tolist(), None if lens is None else lens.tolist()), d, mode, b"##", b" ", skip)
                for dev in (False, True):
                    rc, n, unk, out, off = _call(gpu, objects[which], block=block, lengths=lens, skip=skip, dev=dev)
                    assert rc == _lib.OK and unk == unknown and out == b"".join(want), (n_rows, L, which, dev)
                    assert np.array_equal(off, np.cumsum([0] + [len(w) for w in want]))
    for bad in ([3, 8], [-1, 2]):
        rc, n, unk, out, off = _call(gpu, objects["wp"], block=np.zeros((2, 7), np.int32), lengths=np.array(bad, np.int32), cap=64, dev=bad[0] < 0)
        assert rc == _lib.ERR_INVALID and "length" in _lib.last_error() and n == 0 and (off == -7).all()


def test_the_lds_window(gpu):
    from latok_amd import _lib, batch
    block, win, _, _, lane = _limits()
    sizes = [1, lane - 1, lane, lane + 1, win - 1, win, win + 1, 3 * win + 5, 0, 2, 17]
    words = [bytes((7 * i + j) % 251 for j in range(n)) for i, n in enumerate(sizes)] + [b"##" + bytes((3 * j) % 250 for j in range(win))]
    d = ref.id_map(words)
    rows = [[0, 4, 0], [5], [6, 0], [7, 1, 2, 3], [], [11, 11, 0], [0] * (block + 5), [9, 10, 8, 9]]
    with batch.Detokenizer(words) as concat, batch.Detokenizer(words, mode="wordpiece", prefix=b"##", sep=b"\x00") as wp:
        for phase in range(16):
            _check(gpu, concat, d, rows, ref.CONCAT, dev=True, phase=phase)
            _check(gpu, wp, d, rows[phase % len(rows):] + rows[:phase % len(rows)], ref.WORDPIECE, sep=b"\x00", dev=True, phase=phase)
        _check(gpu, concat, d, rows, ref.CONCAT, dev=False, phase=3)
        _check(gpu, wp, d, rows, ref.WORDPIECE, sep=b"\x00", dev=False, i32=True)
    one_byte = [bytes([b]) for b in range(256)]
    with batch.Detokenizer(one_byte) as detok:
        rng = random.Random(5)
        rows = [[rng.randrange(256) for _ in range(rng.choice((0, 1, 3, 40)))] for _ in range(60)]
        for phase in (0, 1, 15):
            _check(gpu, detok, ref.id_map(one_byte), rows, ref.CONCAT, dev=True, phase=phase)


def test_the_capacity_protocol(gpu, objects):
    from latok_amd import _lib
    d = ref.id_map(WP_WORDS)
    rows = [[1, 3, 4, 5, 2], [], [14, 15, 16, 99], [3]]
    want, unknown = ref.decode(rows, d, ref.WORDPIECE, skip=(1, 2))
    need, want_off = sum(map(len, want)), np.cumsum([0] + [len(w) for w in want])
    for dev in (False, True):
        for kw in (dict(rows=rows), dict(block=np.array([r + [0] * (5 - len(r)) for r in rows], np.int32), lengths=[len(r) for r in rows])):
            rc, n, unk, out, off = _call(gpu, objects["wp"], skip=(1, 2), dev=dev, query=True, **kw)            # the size query
            assert rc == _lib.ERR_INVALID and n == need and unk == unknown and np.array_equal(off, want_off)
            rc, n, unk, out, off = _call(gpu, objects["wp"], skip=(1, 2), dev=dev, cap=need - 1, **kw)          # one byte short
            assert rc == _lib.ERR_INVALID and "need %d bytes" % need in _lib.last_error() and n == need and out == b"" and np.array_equal(off, want_off)
            rc, n, unk, out, off = _call(gpu, objects["wp"], skip=(1, 2), dev=dev, cap=need, **kw)              # exact
            assert rc == _lib.OK and n == need and out == b"".join(want) and np.array_equal(off, want_off)
        rc, n, unk, out, off = _call(gpu, objects["wp"], rows=[[1], [2, 99]], skip=(1, 2), dev=dev, query=True)   # nothing to write: a query that is OK
        assert rc == _lib.OK and n == 0 and unk == 1 and (off == 0).all()
        rc, n, unk, out, off = _call(gpu, objects["wp"], rows=[], dev=dev, cap=8)
        assert rc == _lib.OK and n == 0 and off.tolist() == [0]


def test_malformed_rows_are_refused_and_nothing_is_written(gpu, objects):
    from latok_amd import _lib
    ids = np.arange(6, dtype=np.int32)
    for indptr, needle in (([1, 3, 6], "indptr[0]"), ([0, 4, 3, 6], "non-decreasing"), ([0, 3, 5], "nnz"), ([0, 3, 7], "nnz")):
        for dev in (False, True):
            for i32 in (False, True):
                rc, n, unk, out, off = _call(gpu, objects["concat"], indptr=np.array(indptr, np.int64), ids=ids, dev=dev, i32=i32, cap=256)
                assert rc == _lib.ERR_INVALID and needle in _lib.last_error() and n == 0 and out == b"" and (off == -7).all(), (indptr, dev, i32)
    rc, n, unk, out, off = _call(gpu, objects["concat"], rows=[[3, 4]], cap=64)      # the context still works
    assert rc == _lib.OK and out == b"un##aff"


def test_unknown_ids_and_the_python_calls(gpu, objects):
    from latok_amd import batch
    d = ref.id_map(WP_WORDS)
    rows = [[1, 3, 4, 5, 2, 0, 0], [99, 3, -4, 15], [], [77]]
    out, off = batch.decode_csr(objects["wp"], [0, 7, 11, 11, 12], [i for r in rows for i in r], skip_ids=(0, 1, 2), errors="ignore")
    want, unknown = ref.decode(rows, d, ref.WORDPIECE, skip=(0, 1, 2))
    assert unknown == 3 and out.tobytes() == b"".join(want) == b"unaffableuns" and off.tolist() == [0, 9, 12, 12, 12]
    with pytest.raises(ValueError, match="3 ids"):
        batch.decode_csr(objects["wp"], [0, 7, 11, 11, 12], [i for r in rows for i in r], skip_ids=(0, 1, 2))
    with pytest.raises(ValueError, match="1 ids"):
        batch.decode_batch(objects["concat"], [[3], [1000]])
    assert batch.decode_batch(objects["wp"], rows[:1] + [[14, 16]], skip_ids=[0, 1, 2]) == [b"unaffable", b"the q"]
    assert batch.decode_batch(objects["concat"], np.array([[3, 4, 0], [10, 0, 0]], np.int32), skip_ids=(0,)) == [b"un##aff", b"x"]
    assert batch.decode_batch(objects["concat"], []) == [] and batch.decode_batch(objects["concat"], [[], []]) == [b"", b""]
    block = np.array([[1, 3, 15, 2, 0, 0], [1, 14, 2, 0, 0, 0]], np.int32)
    for kw in (dict(lengths=[4, 3]), dict(attention_mask=(block != 0).astype(np.int32))):
        out, off = batch.decode_padded(objects["wp"], block, skip_ids=(1, 2), **kw)
        assert out.tobytes() == b"unsthe" and off.tolist() == [0, 3, 6]
    i32 = batch.decode_csr(objects["concat"], np.array([0, 2], np.int32), [3, 4])
    assert i32[0].tobytes() == b"un##aff" and i32[1].dtype == np.int64


@pytest.mark.parametrize("lead_space", [0, 1])
def test_round_trip_through_the_bpe_encoder(gpu, lead_space):
    from latok_amd import batch
    rng = random.Random(21 + lead_space)
    texts = [t for name in ("mixed", "words", "latin1") for t in random_strings(rng, 40, 0, 60, ALPHABETS[name])]
    blobs = [t.encode("utf-8") for t in texts]
    merges = bpe_ref.train([w for b in blobs for w in b.split()], 60, base=list(range(256)))
    bos, eos, pad = len(merges), len(merges) + 1, len(merges) + 2
    with batch.BPE(merges, lead_space=bool(lead_space)) as bpe, batch.Detokenizer(merges) as detok:
        indptr, ids, spans = batch.bpe_ids_utf8_batch(blobs, bpe)
        want = [b"".join(blobs[s][a:e] for a, e in spans[indptr[s]:indptr[s + 1]].tolist()) for s in range(len(blobs))]
        assert any(b" " in w for w in want) == bool(lead_space)
        assert batch.decode_batch(detok, [ids[indptr[s]:indptr[s + 1]] for s in range(len(blobs))]) == want
        out, off = batch.decode_csr(detok, indptr.astype(np.int32), ids)
        assert out.tobytes() == b"".join(want)
        for L in (8, 40):
            input_ids, mask = batch.bpe_encode_utf8_batch(blobs, bpe, L, bos_id=bos, eos_id=eos, pad_id=pad)
            cut = [b"".join(blobs[s][a:e] for a, e in spans[indptr[s]:indptr[s + 1]][:L - 2].tolist()) for s in range(len(blobs))]
            assert batch.decode_batch(detok, input_ids, skip_ids=(bos, eos, pad)) == cut
            out, off = batch.decode_padded(detok, input_ids, attention_mask=mask, skip_ids=(bos, eos))
            assert [out.tobytes()[off[s]:off[s + 1]] for s in range(len(blobs))] == cut


def test_round_trip_through_the_wordpiece_encoder(gpu):
    from latok_amd import batch
    rng = random.Random(31)
    texts = [t for name in ("mixed", "words", "starts") for t in random_strings(rng, 40, 0, 60, ALPHABETS[name])]
    blobs = [t.encode("utf-8") for t in texts]
    chars = sorted({c for t in texts for c in t if not c.isspace()})
    # (a prefix no text holds: with "##" a token that IS a continuation word, "##a", would decode without its separator)
    pre = "\x01"
    words = ["[PAD]", "[CLS]", "[SEP]"] + chars + [pre + c for c in chars] + ["ab", pre + "bc", pre + "c", "http", pre + "://"]
    with batch.WordPiece(words, prefix=pre) as wp, batch.Detokenizer(words, mode="wordpiece", prefix=pre) as detok:
        indptr, ids, _ = batch.wordpiece_ids_utf8_batch(blobs, wp, unk_id=-1)
        assert (ids >= 0).all(), "the vocabulary cuts every token into known pieces"
        want = batch.join_tokens_utf8_batch(blobs, sep=b" ")
        assert batch.decode_batch(detok, [ids[indptr[s]:indptr[s + 1]] for s in range(len(blobs))]) == want
        d = ref.id_map([w.encode("utf-8") for w in words])
        for L in (6, 48):
            input_ids, mask = batch.wordpiece_encode_utf8_batch(blobs, wp, L, cls_id=1, sep_id=2, pad_id=0)
            cut = [ref.decode_row(ids[indptr[s]:indptr[s + 1]][:L - 2].tolist(), d, ref.WORDPIECE, pre.encode())[0] for s in range(len(blobs))]
            assert batch.decode_batch(detok, input_ids, skip_ids=(0, 1, 2)) == cut
            out, off = batch.decode_padded(detok, input_ids, lengths=mask.sum(axis=1), skip_ids=(1, 2))
            assert [out.tobytes()[off[s]:off[s + 1]] for s in range(len(blobs))] == cut


def test_two_contexts_decode_with_one_object_at_once_and_destroy_follows_the_last_call(gpu):
    from latok_amd import _lib, batch
    d = ref.id_map(WP_WORDS)
    detok = batch.Detokenizer(WP_WORDS, mode="wordpiece")
    rng = random.Random(9)
    jobs = []
    for k in range(2):
        rows = _rows_of(rng, 700 + 300 * k, list(range(len(WP_WORDS))) + [500], "short")
        jobs.append((rows, ref.decode(rows, d, ref.WORDPIECE, skip=(0,))))
    errors, gate = [], threading.Barrier(2, timeout=60)
    ctxs = [_lib.Context(0) for _ in jobs]

    def run(k):
        try:
            with ctxs[k]:
                gate.wait()
                rows, (want, unknown) = jobs[k]
                for rnd in range(6):
                    got = batch.decode_batch(detok, rows, skip_ids=(0,), errors="ignore")
                    assert got == want, (k, rnd)
        except BaseException as exc:   # noqa: BLE001 - reported to the main thread
            errors.append(exc)
            gate.abort()

    ths = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(120)
    alive = [t.is_alive() for t in ths]
    for ctx, t in zip(ctxs, ths):
        if not t.is_alive():
            ctx.destroy()
    assert not errors and not any(alive), errors
    # destroy behind a call whose device-pointer outputs were just enqueued and waited for: the drain finds nothing to wait for, the object goes
    rows, (want, _) = jobs[0]
    rc, n, unk, out, off = _call(gpu, detok, rows=rows, skip=(0,), dev=True)
    assert rc == _lib.OK and out == b"".join(want)
    detok.close()
    assert detok.handle is None
    with pytest.raises(ValueError, match="detok"):
        batch.decode_batch(detok, [[1]])
