"""Case folding and accent stripping on the device (latok_fold_utf8_bytes_batch, include/latok_hip.h).

Every case is compared in full with tests/helpers/fold_ref.py, the definition restated in plain Python over bytes: n_out_bytes, every
out_off, every output byte, and 64 poison guard bytes behind the end.  The shapes are the smallest at which the kernels can go
wrong: all code points, every alignment of every kind of image against the 16-byte load edge and the tile edge (the tile size is
read from latok_debug_fold_limits), sequences cut by a string end, more strings than bytes in a tile, empty rows, the largest
growth, the capacity protocol and device pointers."""
import ctypes as C

import numpy as np
import pytest

from helpers import fold_ref as ref
from helpers import utf8_cases as cases

pytestmark = pytest.mark.gpu

POISON = 0xA5
GUARD = 64
FOLD_ROUTE = 13
SOFT = [b"ab\xe6\x97 cd", b"\xc3 x", b"lone \xf0\x9f\x98", b"end\xe6", b"next starts ascii", b"\xe6\x97\xa5\xe6", b"\xf0", b"x\xc3"]
HARD = [b"a\x80\x80\x80\x80b", b"\xa9 starts with a continuation byte"]


def _pack(blobs):
    from latok_amd import batch
    return batch.pack_utf8(blobs)


def _fold_host(lib, u8, boff, fold, cap=None, out=True, total=None):
    """the blocking call with host pointers -> (rc, n, out incl. guard bytes, out_off)"""
    n_str = boff.size - 1
    real = int(boff[-1]) if n_str > 0 else 0
    total = real if total is None else total
    cap = 3 * real if cap is None else cap
    buf = np.full(cap + GUARD, POISON, np.uint8)
    off = np.full(n_str + 1, -7, np.int64)
    n = C.c_int64(-1)
    u8 = np.ascontiguousarray(u8)
    rc = lib.latok_fold_utf8_bytes_batch(u8.ctypes.data if u8.size else None, boff.ctypes.data, n_str, total, fold, buf.ctypes.data if out else None,
                                         cap, off.ctypes.data, C.byref(n), 0, None)
    return rc, n.value, buf, off


def _check(lib, u8, boff, fold, what, want=None):
    from latok_amd import _lib
    want_bytes, want_off = ref.fold_batch(u8, boff, fold) if want is None else want
    rc, n, buf, off = _fold_host(lib, u8, boff, fold)
    assert rc == 0, (what, fold, _lib.last_error())
    assert int(boff[-1]) == 0 or lib.latok_debug_last_route() == FOLD_ROUTE
    assert n == want_bytes.size, (what, fold, n, want_bytes.size)
    assert np.array_equal(off, want_off), (what, fold, "out_off", int(np.nonzero(off != want_off)[0][0]))
    if not np.array_equal(buf[:n], want_bytes):
        i = int(np.nonzero(buf[:n] != want_bytes)[0][0])
        raise AssertionError((what, fold, "byte", i, buf[max(i - 8, 0):i + 8].tobytes(), want_bytes[max(i - 8, 0):i + 8].tobytes()))
    assert (buf[n:] == POISON).all(), (what, fold, "guard")


def _tile(lib):
    fn = lib.latok_debug_fold_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(3, np.int64)
    assert fn(out.ctypes.data, 3) == 3
    return int(out[0])


# ---- every code point ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scalars():
    """all 0x110000 code points as one stream, the byte position of every code point, and per combination the reference's bytes and
    out_off of the batch that holds one code point per string (computed once: a batch cut between code points folds to the same
    bytes, and its rows start where those one-code-point rows start)"""
    u8 = cases.all_scalars_stream()
    starts = np.flatnonzero((u8 & 0xC0) != 0x80).astype(np.int64)
    assert starts.size == 0x110000
    return u8, starts, {fold: ref.fold_batch(u8, np.append(starts, np.int64(u8.size)), fold) for fold in ref.COMBOS}


@pytest.mark.parametrize("per_string", [1, 7, 4096])
def test_every_code_point_under_every_combination(gpu, scalars, per_string):
    u8, starts, per_cp = scalars
    boff = np.append(starts[::per_string], np.int64(u8.size))
    for fold in ref.COMBOS:
        want_bytes, cum = per_cp[fold]
        _check(gpu, u8, boff, fold, "scalars/%d" % per_string, (want_bytes, np.append(cum[:-1][::per_string], cum[-1])))


# ---- every alignment, every tile edge --------------------------------------------------------------------------------------
KINDS = [("É", ref.UNCASED), ("Ⱥ", ref.LOWER), ("K", ref.LOWER), ("각", ref.STRIP_MARKS), ("\U0001d160", ref.STRIP_MARKS),
         ("́", ref.STRIP_MARKS), ("日", ref.CJK_SPACE)]


def test_every_kind_of_image_at_every_alignment_and_tile_edge(gpu):
    T = _tile(gpu)
    assert [len(ref.fold_bytes(c.encode(), f)) - len(c.encode()) for c, f in KINDS] == [-1, 1, -2, 6, 8, -2, 2]
    chars = "".join(c for c, _ in KINDS).encode()
    pad = (b"Ab cD,e " * (T // 8 + 4))
    blobs = [pad[:p] + chars + b"Z" for p in range(T + 17)]
    u8, boff = _pack(blobs)
    for fold in (ref.UNCASED, ref.ALL, ref.CJK_SPACE):
        _check(gpu, u8, boff, fold, "alignment")
    # the same characters as one string each, so that every image also starts and ends a row at every alignment
    parts = [x for p in range(0, T + 17, 5) for x in [pad[:p]] + [c.encode() for c, _ in KINDS]]
    u8, boff = _pack(parts)
    _check(gpu, u8, boff, ref.ALL, "alignment/rows")


# ---- the per-string rule ---------------------------------------------------------------------------------------------------
def test_a_sequence_does_not_cross_its_strings_end(gpu):
    from latok_amd import batch
    U = batch.FOLD_UNCASED
    assert batch.fold_utf8_batch([b"x\xc3", b"\xa9y"], U) == [b"x\xc3", b"\xa9y"]
    assert batch.fold_utf8_batch([b"x\xc3\x89y"], U) == [b"xey"]
    assert batch.fold_utf8_batch([b"\xc1\x81"], batch.FOLD_LOWER) == [b"a"] and batch.fold_utf8_batch([b"\xc1\x81"], 0) == [b"\xc1\x81"]
    got = batch.fold_utf8_batch(SOFT + HARD, U)
    assert got == [bytes(b + 32 if 0x41 <= b <= 0x5A else b for b in blob) for blob in SOFT + HARD]
    assert batch.fold_batch(["Unaffable", "ÜNAFFABLE", "İ", "ΟΔΟΣ"]) == ["unaffable", "unaffable", "i", "οδοσ"]
    # string starts on the lead and on every continuation byte of 1-, 2-, 3- and 4-byte chars, at every offset of a 16-byte group
    u8, boff = cases.string_start_case()
    for fold in ref.COMBOS:
        _check(gpu, u8, boff, fold, "string starts")
    # every sequence, cut and uncut, at the dword, group, wave and tile edges; one string per segment and one string per 5 bytes
    u8, boff = cases.edge_stream()
    _check(gpu, u8, boff, ref.ALL, "edges")
    _check(gpu, u8, cases.cut_every(u8.size, 5), ref.UNCASED, "edges/5")
    for u8, boff in cases.tiny_batches():
        _check(gpu, u8, boff, ref.ALL, "tiny")
    # every lead byte with every second byte, one ASCII byte behind: windows that decode to anything
    w = cases.window_stream()[:5 * 64 * 256 * 12]
    _check(gpu, w, cases.cut_every(w.size, 4099), ref.ALL, "windows")


# ---- batch shapes ----------------------------------------------------------------------------------------------------------
def test_batch_shapes(gpu):
    from latok_amd import _lib
    T = _tile(gpu)
    A = ref.ALL
    _check(gpu, *_pack(["Één Straße".encode()]), A, "n_str = 1")
    _check(gpu, *_pack([bytes([65 + i % 26]) for i in range(5000)]), A, "one-byte strings")
    assert 5000 > T
    body = ["Çà et là".encode(), b"", b"", "ВСЁ".encode(), b"", "각" .encode() * 700, b""]
    _check(gpu, *_pack([b"", b""] + body + [b"", b"", b""]), A, "empty strings")
    marks = "̧́̈".encode() * 500
    u8, boff = _pack([b"a", marks, b"b", marks + marks])
    _check(gpu, u8, boff, ref.STRIP_MARKS, "marks only")
    rc, n, _, off = _fold_host(gpu, u8, boff, ref.STRIP_MARKS)
    assert n == 2 and off.tolist() == [0, 1, 1, 2, 2]
    # the largest growth: Hangul LVT syllables only, 3 bytes -> 9
    lvt = "".join(chr(ref.S_BASE + 28 * (k % 399) + 1 + k % 27) for k in range(3000)).encode()
    u8, boff = _pack([lvt[:3 * 1000], lvt[3 * 1000:]])
    rc, n, buf, off = _fold_host(gpu, u8, boff, ref.STRIP_MARKS)
    assert rc == 0 and n == 3 * u8.size and off[-1] == 3 * int(boff[-1])
    _check(gpu, u8, boff, ref.STRIP_MARKS, "hangul")
    # the most a tile can give: T - 1 bytes of LVT syllables, then a lead byte on the tile's last byte whose image has 12 bytes
    assert (T - 1) % 3 == 0
    _check(gpu, *_pack([lvt[:T - 1] + "\U0001d160".encode() * 3 + lvt[:T]]), ref.STRIP_MARKS, "fullest tile")
    # total_bytes = -1
    u8, boff = _pack(["Crème Brûlée".encode(), b"x" * (T + 3), "ǅ".encode()])
    want_bytes, want_off = ref.fold_batch(u8, boff, A)
    rc, n, buf, off = _fold_host(gpu, u8, boff, A, total=-1)
    assert rc == 0 and n == want_bytes.size and np.array_equal(off, want_off) and np.array_equal(buf[:n], want_bytes) and (buf[n:] == POISON).all()
    # n_str = 0, and strings without a byte
    n0 = C.c_int64(-1)
    assert gpu.latok_fold_utf8_bytes_batch(None, np.zeros(1, np.int64).ctypes.data, 0, 0, A, None, 0, None, C.byref(n0), 0, None) == 0 and n0.value == 0
    rc, n, buf, off = _fold_host(gpu, np.zeros(0, np.uint8), np.zeros(4, np.int64), A, cap=8)
    assert rc == 0 and n == 0 and off.tolist() == [0, 0, 0, 0] and (buf == POISON).all(), _lib.last_error()


def test_identity(gpu):
    from latok_amd import batch
    u8, boff = cases.string_start_case()
    out, off = batch.fold_utf8_csr(u8, boff, 0)
    assert np.array_equal(out, u8[:int(boff[-1])]) and np.array_equal(off, boff)
    w = cases.window_stream()[:200000]
    out, off = batch.fold_utf8_csr(w, cases.cut_every(w.size, 777), 0)
    assert np.array_equal(out, w) and np.array_equal(off, cases.cut_every(w.size, 777))


# ---- the capacity protocol -------------------------------------------------------------------------------------------------
def test_capacity_protocol(gpu):
    from latok_amd import _lib
    blobs = ["Ünï Çödé 각 日本".encode() * 40, b"", "ÀÉÎ".encode() * 1500]
    u8, boff = _pack(blobs)
    want_bytes, want_off = ref.fold_batch(u8, boff, ref.ALL)
    need = want_bytes.size
    rc, n, buf, off = _fold_host(gpu, u8, boff, ref.ALL, cap=need - 1)
    assert rc == _lib.ERR_INVALID and "need %d bytes" % need in _lib.last_error()
    assert n == need and np.array_equal(off, want_off) and (buf == POISON).all()
    rc, n, buf, off = _fold_host(gpu, u8, boff, ref.ALL, cap=0, out=False)                  # a size query
    assert rc == _lib.ERR_INVALID and n == need and np.array_equal(off, want_off)
    rc, n, buf, off = _fold_host(gpu, u8, boff, ref.ALL, cap=need)
    assert rc == 0 and n == need and np.array_equal(buf[:n], want_bytes) and (buf[n:] == POISON).all()
    rc, n, buf, off = _fold_host(gpu, u8, boff, ref.ALL, cap=16, out=False)
    assert rc == _lib.ERR_INVALID and "out_bytes is NULL" in _lib.last_error()


# ---- device pointers -------------------------------------------------------------------------------------------------------
def test_device_pointers_equal_host_pointers(gpu):
    from latok_amd import _lib
    u8, boff = cases.string_start_case()
    fold = ref.ALL
    rc, need, want_buf, want_off = _fold_host(gpu, u8, boff, fold)
    assert rc == 0
    sizes = (u8.nbytes + 128, boff.nbytes, need + GUARD, boff.nbytes)
    ptrs = [gpu.latok_dev_alloc(s) for s in sizes]
    assert all(ptrs) and all(p % 16 == 0 for p in ptrs)
    d_u8, d_boff, d_out, d_off = ptrs
    try:
        _lib.check(gpu.latok_memcpy_h2d(d_u8, u8.ctypes.data, u8.nbytes))
        _lib.check(gpu.latok_memcpy_h2d(d_boff, boff.ctypes.data, boff.nbytes))
        _lib.check(gpu.latok_memset_dev(d_out, POISON, need + GUARD))
        _lib.check(gpu.latok_sync())
        n = C.c_int64(-1)
        rc = gpu.latok_fold_utf8_bytes_batch(d_u8, d_boff, boff.size - 1, -1, fold, d_out, need, d_off, C.byref(n), _lib.DEVICE_PTRS, None)
        assert rc == 0 and n.value == need, _lib.last_error()
        buf, off = np.empty(need + GUARD, np.uint8), np.empty(boff.size, np.int64)
        _lib.check(gpu.latok_memcpy_d2h(buf.ctypes.data, d_out, buf.nbytes))
        _lib.check(gpu.latok_memcpy_d2h(off.ctypes.data, d_off, off.nbytes))
        assert np.array_equal(buf[:need], want_buf[:need]) and (buf[need:] == POISON).all() and np.array_equal(off, want_off)
        # too small: nothing is written, the need and the offsets are reported
        _lib.check(gpu.latok_memset_dev(d_out, POISON, need + GUARD))
        rc = gpu.latok_fold_utf8_bytes_batch(d_u8, d_boff, boff.size - 1, -1, fold, d_out, need - 1, d_off, C.byref(n), _lib.DEVICE_PTRS, None)
        assert rc == _lib.ERR_INVALID and n.value == need
        _lib.check(gpu.latok_memcpy_d2h(buf.ctypes.data, d_out, buf.nbytes))
        assert (buf == POISON).all()
        # an unaligned device input is refused
        rc = gpu.latok_fold_utf8_bytes_batch(d_u8 + 4, d_boff, boff.size - 1, int(boff[-1]), fold, d_out, need, d_off, C.byref(n), _lib.DEVICE_PTRS, None)
        assert rc == _lib.ERR_INVALID and "16-byte aligned" in _lib.last_error()
    finally:
        for p in ptrs:
            gpu.latok_dev_free(p)


# ---- a corpus --------------------------------------------------------------------------------------------------------------
def test_mixed_unicode_corpus(gpu):
    from latok_amd import _lib
    n_str = 2000
    row = np.zeros(n_str + 1, np.int64)
    _lib.check(gpu.latok_corpus_offsets(2024, 0, n_str, 64, 256, row.ctypes.data))
    cps = np.zeros(int(row[-1]), np.uint32)
    _lib.check(gpu.latok_corpus_fill_host(2024, _lib.CORPUS_UNICODE, 0, n_str, row.ctypes.data, cps.ctypes.data))
    blobs = [cps[row[s]:row[s + 1]].astype("<u4").tobytes().decode("utf-32-le", "surrogatepass").encode("utf-8", "surrogatepass") for s in range(n_str)]
    u8, boff = _pack(blobs)
    assert (u8 >= 0x80).mean() > 0.05
    for fold in (ref.UNCASED, ref.ALL):
        _check(gpu, u8, boff, fold, "corpus")
