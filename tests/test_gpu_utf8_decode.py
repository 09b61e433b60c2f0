"""Every UTF-8 decode route of the library against one independent reference (tests/helpers/utf8_ref.py: the rule of
include/latok_hip.h restated in plain Python): the staged device decoder (latok_utf8_decode_batch) on every window, every sequence
at every edge of dword, chunk, wave and block, every string start, all scalar values and a batch above the big scan's threshold,
through host pointers, aligned and shifted device pointers; and the calls that delegate to it or to the host decoder or to byte
space (split_mask / split_offsets / token_spans / token_features of UTF-8 in code-point units), route by route.  All comparisons are
exact; no input is filtered.  tests/test_utf8_decode_host.py proves without a device what the streams reach."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from conftest import ALPHABETS, RULE_SETS, random_strings
from helpers import utf8_cases as cases
from helpers import utf8_ref as ref
from test_gpu_features_utf8 import _oracle_raw
from test_utf8_decode_host import decode_limits

pytestmark = pytest.mark.gpu

POISON, ROW_POISON, GUARD = 0xA5A5A5A5, -7, 8
DTYPES = (np.int64, np.int32)
EXTRA = list("é日🤓ü　Жδ") + ["http://a.b/c?d=1", "see me@x.org", "#tag", ".@you", "a@b.c"]


def _small_chars():
    from test_host_api import debug_limits
    return debug_limits()["kSmallChars"]


def _route():
    from latok_amd import _lib
    return _lib.load().latok_debug_last_route()


# ---- latok_utf8_decode_batch with poisoned outputs and guard words ------------------------------------------------------------
def _decode(lib, u8, boff, total=None, cap=None, dev=False, shift=0):
    """-> (rc, total_cps_out, cps_out with GUARD words behind cap, cp_row_off_out with GUARD words behind it); dev: every pointer
    is a device pointer, the bytes at a 16-byte aligned address + shift"""
    from latok_amd import _lib
    u8 = np.ascontiguousarray(u8, np.uint8)
    boff = np.ascontiguousarray(boff, np.int64)
    n_str = boff.size - 1
    nbytes = int(boff[-1]) if n_str > 0 else 0
    total = nbytes if total is None else total
    cap = nbytes if cap is None else cap
    cps = np.full(cap + GUARD, POISON, np.uint32)
    row = np.full(n_str + 1 + GUARD, ROW_POISON, np.int64)
    n = C.c_int64(-1)
    if not dev:
        rc = lib.latok_utf8_decode_batch(u8.ctypes.data if nbytes else None, boff.ctypes.data, n_str, total, cps.ctypes.data, cap,
                                         row.ctypes.data, C.byref(n), 0, None)
        return rc, n.value, cps, row
    d_u8, d_boff = lib.latok_dev_alloc(nbytes + 64), lib.latok_dev_alloc(boff.nbytes)
    d_cps, d_row = lib.latok_dev_alloc(cps.nbytes), lib.latok_dev_alloc(row.nbytes)
    assert d_u8 and d_boff and d_cps and d_row and d_u8 % 16 == 0
    try:
        if nbytes:
            _lib.check(lib.latok_memcpy_h2d(d_u8 + shift, u8.ctypes.data, nbytes))
        _lib.check(lib.latok_memcpy_h2d(d_boff, boff.ctypes.data, boff.nbytes))
        _lib.check(lib.latok_memcpy_h2d(d_cps, cps.ctypes.data, cps.nbytes))
        _lib.check(lib.latok_memcpy_h2d(d_row, row.ctypes.data, row.nbytes))
        rc = lib.latok_utf8_decode_batch(d_u8 + shift, d_boff, n_str, total, d_cps, cap, d_row, C.byref(n), _lib.DEVICE_PTRS, None)
        _lib.check(lib.latok_memcpy_d2h(cps.ctypes.data, d_cps, cps.nbytes))
        _lib.check(lib.latok_memcpy_d2h(row.ctypes.data, d_row, row.nbytes))
        return rc, n.value, cps, row
    finally:
        for p in (d_u8, d_boff, d_cps, d_row):
            lib.latok_dev_free(p)


def _first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return None if bad.size == 0 else (int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])), int(bad.size))


def _check_decode(lib, u8, boff, want=None, what="", **kw):
    """the call succeeds and gives the reference's cps, rows and total; nothing is written behind them"""
    boff = np.asarray(boff, np.int64)
    w_cps, w_row, w_total = ref.decode_batch(u8, boff) if want is None else want
    rc, n, cps, row = _decode(lib, u8, boff, **kw)
    assert rc == 0 and n == w_total, (what, rc, n, w_total)
    assert _first_difference(cps[:n], w_cps) is None, (what, "cps", _first_difference(cps[:n], w_cps))
    assert _first_difference(row[:boff.size], w_row) is None, (what, "cp_row_off", _first_difference(row[:boff.size], w_row))
    assert (cps[n:] == POISON).all() and (row[boff.size:] == ROW_POISON).all(), (what, "written behind the results")


@functools.lru_cache(maxsize=None)
def _window_case():
    u8 = cases.window_stream()
    cps, lead = ref.decode_per_lead(u8)
    for a in (u8, cps, lead):
        a.setflags(write=False)
    return u8, cps, lead


@functools.lru_cache(maxsize=None)
def _scalars_case(prefix):
    u8 = cases.all_scalars_stream(prefix)
    cps, lead = ref.decode_per_lead(u8)
    for a in (u8, cps, lead):
        a.setflags(write=False)
    return u8, cps, lead


def _rows(lead, boff):
    return np.searchsorted(lead, boff, side="left").astype(np.int64)


# ---- (a) every window ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [0, 7])
def test_every_window(gpu, cut):
    """every lead byte 0xC0..0xFF with every second byte and third / fourth bytes over both ends of the continuation range and
    bytes outside it, at every phase of dword, chunk, wave and block; as one string, and as strings of 7 bytes that open with
    continuation bytes and cut sequences"""
    u8, cps, lead = _window_case()
    boff = cases.cut_every(u8.size, cut) if cut else np.array([0, u8.size], np.int64)
    _check_decode(gpu, u8, boff, want=(cps, _rows(lead, boff), int(cps.size)), what=cut)


# ---- (b) every sequence at every edge --------------------------------------------------------------------------------------
def test_every_sequence_at_every_edge(gpu):
    u8, boff = cases.edge_stream()
    _check_decode(gpu, u8, boff, what="filler behind")
    _check_decode(gpu, u8, np.array([0, u8.size], np.int64), what="filler behind, one string")


def test_every_sequence_cut_by_the_end_of_the_batch(gpu):
    """the batch ends 0..3 bytes behind a lead byte that sits 0..4 bytes in front of every edge: a call per case"""
    n = 0
    for data, pos in cases.end_of_batch_cases():
        u8 = np.frombuffer(data, np.uint8)
        _check_decode(gpu, u8, np.array([0, u8.size], np.int64), what=(data[pos:], pos))
        if pos > 0:
            _check_decode(gpu, u8, np.array([0, pos, pos, u8.size], np.int64), what=(data[pos:], pos, "own string"))
        n += 1
    assert n >= 16 * 25


# ---- (c) string starts -----------------------------------------------------------------------------------------------------
def test_string_starts(gpu):
    u8, boff = cases.string_start_case()
    _check_decode(gpu, u8, boff, what="string starts")
    _check_decode(gpu, u8, boff, what="string starts, device pointers", dev=True)


def test_tiny_batches(gpu):
    n = C.c_int64(-1)
    z = np.zeros(1, np.int64)
    assert gpu.latok_utf8_decode_batch(None, z.ctypes.data, 0, 0, None, 0, None, C.byref(n), 0, None) == 0 and n.value == 0
    empty = np.zeros(0, np.uint8)
    _check_decode(gpu, empty, np.array([0, 0], np.int64), what="one empty string")
    _check_decode(gpu, empty, np.array([0, 0, 0, 0], np.int64), what="three empty strings")
    _check_decode(gpu, empty, np.array([0, 0], np.int64), what="one empty string, device pointers", dev=True)
    for u8, boff in cases.tiny_batches():
        _check_decode(gpu, u8, boff, what=(u8.tobytes(), boff.tolist()))


# ---- (d) all scalar values -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", [0, 1, 2, 3])
def test_all_scalar_values_without_separators(gpu, prefix):
    u8, cps, lead = _scalars_case(prefix)
    assert cps.size == prefix + 0x110000 and np.array_equal(cps[prefix:], np.arange(0x110000, dtype=np.uint32))
    boff = np.array([0, u8.size], np.int64)
    _check_decode(gpu, u8, boff, want=(cps, _rows(lead, boff), int(cps.size)), what=prefix)


# ---- (e) the big scan ------------------------------------------------------------------------------------------------------
def test_batch_above_the_three_launch_scan_threshold(gpu):
    scan_small_max, block = decode_limits()
    u8 = cases.big_stream(scan_small_max * block)
    assert u8.size > scan_small_max * block and (u8.size + block - 1) // block > scan_small_max
    # strings that start in the first and in the last scan block, and on both sides of the threshold
    edge = scan_small_max * block
    boff = np.array([0, 3, block - 1, edge - 1, edge, edge + 1, u8.size - 2, u8.size], np.int64)
    _check_decode(gpu, u8, boff, what="big scan")


# ---- (f) pointer modes and capacity ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pointer_case():
    """string starts, a slice of the windows and the edge placements of two sequences: ~120 KB, more than one wave and block"""
    s_u8, s_off = cases.string_start_case()
    w = cases.window_stream().reshape(-1, 5)[::97].ravel()
    e = np.frombuffer(b"".join(cases.edge_segment(s, d) for s in (b"\xf0\x9f\xa4\x93", b"\xe6\x97") for d in range(-4, 1)), np.uint8)
    u8 = np.concatenate([s_u8, w, e])
    boff = np.concatenate([s_off, s_off[-1] + cases.cut_every(w.size, 11)[1:], [u8.size]]).astype(np.int64)
    want = ref.decode_batch(u8, boff)
    return u8, boff, want


def test_host_and_aligned_device_pointers(gpu):
    u8, boff, want = _pointer_case()
    _check_decode(gpu, u8, boff, want=want, what="host")
    _check_decode(gpu, u8, boff, want=want, what="device", dev=True)
    _check_decode(gpu, u8, boff, want=want, what="host, total_bytes = -1", total=-1)
    _check_decode(gpu, u8, boff, want=want, what="device, total_bytes = -1", dev=True, total=-1)


@pytest.mark.parametrize("shift", list(range(1, 16)))
def test_shifted_device_pointer(gpu, shift):
    """latok_utf8_decode_batch has no alignment rule: a device pointer that is not 16-byte aligned takes the byte-wise loads"""
    u8, boff, want = _pointer_case()
    _check_decode(gpu, u8, boff, want=want, what=shift, dev=True, shift=shift)
    # and a batch that ends inside a chunk, cut short
    tail = np.frombuffer(cases.filler(4096 + 13) + b"\xf0\x9f\xa4", np.uint8)
    _check_decode(gpu, tail, np.array([0, 5, tail.size], np.int64), what=(shift, "cut by the end"), dev=True, shift=shift)


@pytest.mark.parametrize("dev", [False, True])
def test_capacity(gpu, dev):
    from latok_amd import _lib
    u8, boff, want = _pointer_case()
    w_cps, w_row, w_total = want
    rc, n, cps, row = _decode(gpu, u8, boff, cap=w_total - 1, dev=dev)
    assert rc == _lib.ERR_INVALID and n == w_total
    assert (cps == POISON).all(), "cps_out was written although the capacity was refused"
    rc, n, cps, row = _decode(gpu, u8, boff, cap=w_total, dev=dev)
    assert rc == 0 and n == w_total and np.array_equal(cps[:n], w_cps) and np.array_equal(row[:boff.size], w_row)
    assert (cps[n:] == POISON).all() and cps.size == n + GUARD and (row[boff.size:] == ROW_POISON).all()
    rc, n, cps, row = _decode(gpu, u8, boff, cap=0, dev=dev)
    assert rc == _lib.ERR_INVALID and n == w_total and (cps == POISON).all()


# ---- (g) the calls that delegate -------------------------------------------------------------------------------------------
CALLS = ("mask", "offsets", "spans", "features")


def _host_calls(u8, boff, dt, names=CALLS):
    from latok_amd import batch
    out, routes = {}, []
    if "mask" in names:
        out["mask"] = batch.split_mask_utf8_csr(u8, boff)
    for name, fn in (("offsets", batch.split_offsets_utf8_csr), ("spans", batch.token_spans_utf8_csr), ("features", batch.token_features_utf8_csr)):
        if name in names:
            out[name] = fn(u8, boff, dtype=dt)
            routes.append(_route())
    return out, routes


def _dev_calls(lib, u8, boff, dt, shift=0, names=CALLS):
    """the four calls (or those of `names`) with device pointers, the bytes at an aligned address + shift"""
    from latok_amd import _lib
    u8 = np.ascontiguousarray(u8, np.uint8)
    n_str, nbytes = boff.size - 1, int(boff[-1])
    isz = np.dtype(dt).itemsize
    flags = _lib.DEVICE_PTRS | (_lib.OUT_INT32 if dt == np.int32 else 0)
    cap = max(nbytes, 1)
    words = (nbytes + 63) // 64
    sizes = dict(u8=nbytes + 64, boff=boff.nbytes, bits=words * 8 + 16, row=(n_str + 1) * 8, counts=n_str * isz + 16, items=cap * 4 * isz + 16,
                 feats=cap * 25 + 16)
    d = {k: lib.latok_dev_alloc(v) for k, v in sizes.items()}
    assert all(d.values()) and d["u8"] % 16 == 0
    out, routes = {}, []
    try:
        _lib.check(lib.latok_memcpy_h2d(d["u8"] + shift, u8.ctypes.data, nbytes))
        _lib.check(lib.latok_memcpy_h2d(d["boff"], boff.ctypes.data, boff.nbytes))
        n = C.c_int64(-1)
        if "mask" in names:
            _lib.check(lib.latok_split_mask_utf8_batch(d["u8"] + shift, d["boff"], n_str, -1, d["bits"], words, d["row"], C.byref(n), _lib.DEVICE_PTRS, None))
            bits, row = np.zeros((n.value + 63) // 64, np.uint64), np.zeros(n_str + 1, np.int64)
            if bits.size:
                _lib.check(lib.latok_memcpy_d2h(bits.ctypes.data, d["bits"], bits.nbytes))
            _lib.check(lib.latok_memcpy_d2h(row.ctypes.data, d["row"], row.nbytes))
            out["mask"] = (bits, row)
        for name, fn, width in (("offsets", lib.latok_split_offsets_utf8_batch, 1), ("spans", lib.latok_token_spans_utf8_batch, 2),
                                ("features", lib.latok_token_features_utf8_batch, 4)):
            if name not in names:
                continue
            args = [d["u8"] + shift, d["boff"], n_str, -1, d["counts"], d["items"]] + ([d["feats"]] if width == 4 else []) + [cap, C.byref(n), flags, None]
            _lib.check(fn(*args))
            routes.append(_route())
            counts = np.empty(n_str, dt)
            items = np.empty((n.value, width) if width > 1 else n.value, dt)
            _lib.check(lib.latok_memcpy_d2h(counts.ctypes.data, d["counts"], counts.nbytes))
            if items.nbytes:
                _lib.check(lib.latok_memcpy_d2h(items.ctypes.data, d["items"], items.nbytes))
            res = (counts, items)
            if width == 4:
                feats = np.empty((n.value, 25), np.int8)
                if feats.nbytes:
                    _lib.check(lib.latok_memcpy_d2h(feats.ctypes.data, d["feats"], feats.nbytes))
                res += (feats,)
            out[name] = res
        return out, routes
    finally:
        for p in d.values():
            lib.latok_dev_free(p)


def _utf32_calls(cps, row, dt):
    """the expectation: the UTF-32 calls on the REFERENCE's code points and rows"""
    from latok_amd import batch
    cps = np.ascontiguousarray(cps, np.uint32)
    return {"mask": (batch.split_mask_batch(cps, row), row), "offsets": batch.split_offsets_csr(cps, row, dtype=dt),
            "spans": batch.token_spans_csr(cps, row, dtype=dt), "features": batch.token_features_csr(cps, row, dtype=dt)}


def _same_results(got, want, what, names=CALLS):
    for name in names:
        assert len(got[name]) == len(want[name]), (what, name)
        for k, (g, w) in enumerate(zip(got[name], want[name])):
            assert g.shape == w.shape and np.array_equal(g, w), (what, name, k)


def _oracle_results(oracle, cps, row):
    """mask bits, offsets, raw spans and feature sums straight from the oracle, on the reference's code points"""
    texts = [cps[row[i]:row[i + 1]].astype("<u4").tobytes().decode("utf-32-le", "surrogatepass") for i in range(row.size - 1)]
    bits = oracle.split_batch(np.ascontiguousarray(cps, np.uint32), row, want_values=False)[1]
    offs = [oracle.split_offsets(t) if t else np.zeros(0, np.int64) for t in texts]
    return bits, np.array([len(o) for o in offs]), (np.concatenate(offs) if offs else np.zeros(0, np.int64)), _oracle_raw(oracle, texts)


def _check_against_oracle(oracle, got, cps, row, what):
    bits, n_offs, offs, (counts, raw, feats) = _oracle_results(oracle, cps, row)
    assert np.array_equal(got["mask"][0], bits), (what, "mask")
    assert np.array_equal(got["offsets"][0], n_offs) and np.array_equal(got["offsets"][1], offs), (what, "offsets")
    assert np.array_equal(got["spans"][0], counts), (what, "span counts")
    assert np.array_equal(got["features"][0], counts) and np.array_equal(got["features"][1][:, :2], raw), (what, "raw spans")
    assert np.array_equal(got["features"][2], feats), (what, "feature sums")


def _blobs(texts):
    return [t.encode("utf-8", "surrogatepass") for t in texts]


def _pack(blobs):
    from latok_amd import batch
    return batch.pack_utf8(blobs)


SMALL_TEXTS = ["featurize é日🤓 me@x.org http://a.b #tag  ", "", "Ünï ９ .@you", "a@b.c 日本語, ok", " "]
SOFT, HARD = b"ab\xe6\x97 cd \xc3", b"a\x80\x80\x80\x80b \xa9x"


@pytest.mark.parametrize("case", ["host_small", "host_small_malformed", "device_small", "device_small_shifted"])
def test_small_batches_route_by_route_against_the_oracle(gpu, oracle, case):
    blobs = _blobs(SMALL_TEXTS)
    if case == "host_small_malformed":
        blobs = blobs[:2] + [SOFT] + blobs[2:] + [HARD[:6]]
    u8, boff = _pack(blobs)
    cps, row, _ = ref.decode_batch(u8, boff)
    assert cps.max() < 0x110000
    for dt in DTYPES:
        if case.startswith("host"):
            got, routes = _host_calls(u8, boff, dt)
            assert routes == [1 if case == "host_small" else 2] * 3, (case, routes)
        else:
            got, routes = _dev_calls(gpu, u8, boff, dt, shift=5 if case.endswith("shifted") else 0)
            assert routes == [2] * 3, (case, routes)
        _same_results(got, _utf32_calls(cps, row, dt), (case, dt))
        _check_against_oracle(oracle, got, cps, row, (case, dt))


@functools.lru_cache(maxsize=None)
def _large_blobs():
    rng = random.Random(0xDEC0DE)
    return tuple(_blobs([""] + random_strings(rng, 4000, 0, 90, ALPHABETS["mixed"] + EXTRA) + [""]))


@pytest.mark.parametrize("case,route", [("host", 3), ("device", 3), ("device_shifted_4", 2), ("host_hard_malformed", 2),
                                        ("device_hard_malformed", 2), ("host_soft_malformed", 3)])
def test_large_batches_route_by_route(gpu, case, route):
    blobs = list(_large_blobs())
    if "hard" in case:
        blobs[1500:1500] = [SOFT, HARD]
    elif "soft" in case:
        blobs[1500:1500] = [SOFT]
        blobs.append(b"end\xe6")
    u8, boff = _pack(blobs)
    assert u8.size > _small_chars()
    cps, row, _ = ref.decode_batch(u8, boff)
    for dt in DTYPES:
        if case.startswith("host"):
            got, routes = _host_calls(u8, boff, dt)
        else:
            got, routes = _dev_calls(gpu, u8, boff, dt, shift=4 if "shifted" in case else 0)
        assert routes == [route] * 3, (case, routes)
        _same_results(got, _utf32_calls(cps, row, dt), (case, dt))


@functools.lru_cache(maxsize=None)
def _growing_pair():
    """two seeded batches with multi-byte chars -- A: the smallest above kSmallChars bytes (the first that takes route 3), B: about
    twice A -- and A with one stray continuation byte; with every expectation: the UTF-32 calls on the reference's decode"""
    from latok_amd import batch
    from test_gpu_features_utf8_bytes import _to_bytes
    rng = random.Random(0x9A0B)
    blobs = _blobs(random_strings(rng, 12000, 0, 90, ALPHABETS["mixed"] + EXTRA))
    ends = np.cumsum([len(b) for b in blobs])
    n_a, n_b = (int(np.searchsorted(ends, k * _small_chars(), side="right")) + 1 for k in (1, 2))
    assert n_b <= len(blobs)
    odd = blobs[:n_a]
    odd[n_a // 2] = b"\x80" + odd[n_a // 2]
    case = {}
    for key, part in (("A", blobs[:n_a]), ("B", blobs[:n_b]), ("A_odd", odd)):
        u8, boff = _pack(part)
        assert u8.size > _small_chars() and (u8 >= 0x80).any()
        cps, row, _ = ref.decode_batch(u8, boff)
        case[key] = dict(u8=u8, boff=boff, cps=np.ascontiguousarray(cps, np.uint32), row=row)
    assert case["A"]["u8"].size - len(blobs[n_a - 1]) <= _small_chars() and case["B"]["u8"].size < 2 * _small_chars() + 400
    a, b, o = case["A"], case["B"], case["A_odd"]
    want = {("A", "spans"): batch.token_spans_csr(a["cps"], a["row"]), ("A", "mask"): (batch.split_mask_batch(a["cps"], a["row"]), a["row"]),
            ("A", "offsets"): batch.split_offsets_csr(a["cps"], a["row"]), ("B", "features"): batch.token_features_csr(b["cps"], b["row"]),
            ("B", "spans"): batch.token_spans_csr(b["cps"], b["row"], dtype=np.int32), ("A_odd", "spans"): batch.token_spans_csr(o["cps"], o["row"])}
    # featurize in byte space: the same tokens and sums, the records as byte positions (B is well formed: a char's bytes follow from its value)
    counts, spans4, feats = want["B", "features"]
    pos = np.zeros(b["cps"].size + 1, np.int64)
    np.cumsum(1 + (b["cps"] >= 0x80).astype(np.int64) + (b["cps"] >= 0x800) + (b["cps"] >= 0x10000), out=pos[1:])
    assert pos[-1] == b["u8"].size
    want["B", "bytes_features"] = (counts, _to_bytes(spans4, counts, b["row"], pos), feats)
    return case, want


@pytest.mark.parametrize("pointers", ["host", "device"])
def test_calls_of_different_shape_share_one_growing_workspace(gpu, pointers):
    """the blocking code-point calls keep the planes of their byte-space front in the context's workspace, which the compaction
    behind the front sizes again: on a fresh context, calls of different kind and size in turn -- every plane is allocated by one
    call, grown by the next and reused by the one after -- and each result is the UTF-32 call's on the reference's decode"""
    from latok_amd import _lib, batch
    from test_gpu_features_utf8_bytes import _dev_features
    case, want = _growing_pair()
    steps = [("A", "spans", np.int64, 3), ("B", "features", np.int64, 3), ("A", "mask", np.int64, None), ("B", "bytes_features", np.int64, 4),
             ("A", "offsets", np.int64, 3), ("B", "spans", np.int32, 3), ("A_odd", "spans", np.int64, 2), ("A", "spans", np.int64, 3)]
    with _lib.Context(_lib.default_device()):
        for k, (key, name, dt, route) in enumerate(steps):
            u8, boff = case[key]["u8"], case[key]["boff"]
            if name == "bytes_features":
                if pointers == "host":
                    got = {name: batch.token_features_utf8_bytes_csr(u8, boff, dtype=dt)}
                else:
                    rc, n, res, _ = _dev_features(gpu, u8, boff, dt)
                    assert rc == 0 and n == res[1].shape[0], (k, _lib.last_error())
                    got = {name: res}
                routes = [_route()]
            elif pointers == "host":
                got, routes = _host_calls(u8, boff, dt, names=(name,))
            else:
                got, routes = _dev_calls(gpu, u8, boff, dt, names=(name,))
            assert routes == ([] if route is None else [route]), (k, key, name, routes)
            _same_results(got, {name: want[key, name]}, (pointers, k, key, name), names=(name,))


@pytest.mark.parametrize("rules", ["default", "all_columns"])
@pytest.mark.parametrize("n_bytes", [40, 5000, 300000])
def test_lone_lead_bytes_without_any_continuation_byte(gpu, oracle, rules, n_bytes):
    """a batch without continuation bytes skips the decode (byte positions are code-point positions) -- also when it holds lead
    bytes that announce continuation bytes: each of them is U+FFFD in mask, offsets, spans and sums"""
    from latok_amd import batch
    blob = cases.lone_leads_blob(n_bytes, n_bytes)
    if n_bytes == 40:
        assert len(blob) == 40 or blob.startswith(b"a\xc3 b\xff, \xe6 x\xf0")
    assert len(blob) > (0 if n_bytes == 40 else 4096 if n_bytes == 5000 else _small_chars())
    batches = [[blob], [blob[i:i + 97] for i in range(0, len(blob), 97)]]
    # one continuation byte in the whole batch: the decode must not be skipped
    batches += [[blob + "é".encode()], ["é".encode() + blob[:n_bytes // 2], b"", blob[n_bytes // 2:]]]
    if rules != "default":
        batch.set_rules(*RULE_SETS[rules])
    try:
        for k, blobs in enumerate(batches):
            u8, boff = _pack(blobs)
            cps, row, total = ref.decode_batch(u8, boff)
            assert ((cps == ref.REPLACEMENT) == (u8[(u8 & 0xC0) != 0x80] >= 0xC0)).all() or k >= 2
            for dt in DTYPES:
                got, routes = _host_calls(u8, boff, dt)
                assert routes == [2 if u8.size <= _small_chars() else 3] * 3, (k, routes)
                assert got["mask"][1][-1] == total
                _same_results(got, _utf32_calls(cps, row, dt), (rules, n_bytes, k, dt))
                if rules == "default" and n_bytes <= 5000:
                    _check_against_oracle(oracle, got, cps, row, (n_bytes, k, dt))
            if k < 2:
                got, _ = _dev_calls(gpu, u8, boff, np.int64)
                _same_results(got, _utf32_calls(cps, row, np.int64), (rules, n_bytes, k, "device"))
    finally:
        batch.reset_rules()
