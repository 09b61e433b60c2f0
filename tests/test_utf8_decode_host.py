"""The UTF-8 decode rule (include/latok_hip.h: latok_utf8_decode_batch) without a device: the scalar and the numpy reference of
tests/helpers/utf8_ref.py against each other, against Python's own decoder on well-formed input, and against the decoders of
latok_amd/csrc/utf8_decode.h compiled by g++ (utf8_decode_at<0..15>, utf8_decode_bytes, utf8_cp_of, utf8_lead_nibble) on every
window the issue names; the host decoder of small batches (host_decode_small) against the reference; and every byte stream that
tests/test_gpu_utf8_decode.py sends to the device through the scalar reference, with a census that proves what those streams reach."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import utf8_cases as cases
from helpers import utf8_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def decode_limits():
    """entries 15 and 16 of latok_debug_limits (needs no device): kScanSmallMax, kU8Block"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(17, np.int64)
    assert fn(out.ctypes.data, 17) == 17
    return int(out[15]), int(out[16])


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("utf8_decode")
    exe = d / "utf8_decode_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "utf8_decode_harness.cpp"), "-o", str(exe)])

    def run(mode, data, poison=0):
        src, dst = d / "in.bin", d / "out.bin"
        np.ascontiguousarray(data).tofile(str(src))
        subprocess.check_call([str(exe), mode, str(src), str(dst)] + (["%02x" % poison] if mode == "w" else []))
        return np.fromfile(str(dst), np.uint32)

    return run


@pytest.fixture(scope="module")
def all_windows():
    """every window and the numpy reference's value of its first byte (leads only)"""
    w = cases.windows()
    flat = np.concatenate([w, np.full((w.shape[0], 1), 0x20, np.uint8)], axis=1).ravel()     # each window in front of a lead byte
    cps, lead = ref.decode_per_lead(flat)
    first = lead % 5 == 0
    is_lead = (w[:, 0] & 0xC0) != 0x80
    assert np.array_equal(lead[first] // 5, np.flatnonzero(is_lead))
    want = np.zeros(w.shape[0], np.uint32)
    want[is_lead] = cps[first]
    return w, is_lead, want


def test_scalar_and_numpy_reference_agree_on_every_window(all_windows):
    w, is_lead, want = all_windows
    assert w.shape[0] == 256 * 256 * 144
    rows = w.tobytes()
    cp_at = ref.cp_at
    got = [cp_at(rows[4 * i:4 * i + 4], 0) for i in np.flatnonzero(is_lead).tolist()]
    assert np.array_equal(np.array(got, np.uint32), want[is_lead])
    # a window that the end of the batch cuts: the bytes that are missing count as "not a continuation byte"
    for b0 in (0x41, 0xC3, 0xE6, 0xF0, 0xFF):
        for have in range(4):
            data = bytes([b0, 0x97, 0xA5, 0x93][:1 + have])
            want1 = ref.cp_at(data + b"\xff\xff\xff", 0)
            assert ref.cp_at(data, 0) == want1 and ref.decode_per_lead(np.frombuffer(data, np.uint8))[0][0] == want1
            assert (want1 == ref.REPLACEMENT) == (have < ref.n_cont(b0))


def test_device_decoders_compiled_for_the_host_equal_the_reference(harness, all_windows):
    w, is_lead, want = all_windows
    n = w.shape[0]
    multi = w[:, 0] >= 0xC0
    for poison in (0x80, 0xFF, 0x41):        # what lies around the window inside the 19 bytes must not reach the value
        out = harness("w", w, poison)
        lo, hi, by, cp_of = out[:n], out[n:2 * n], out[2 * n:3 * n], out[3 * n:]
        for name, got in (("utf8_decode_at, smallest over I", lo), ("utf8_decode_at, largest over I", hi), ("utf8_decode_bytes", by)):
            bad = np.flatnonzero((got != want) & is_lead)
            assert bad.size == 0, (name, poison, w[bad[0]].tolist(), hex(got[bad[0]]), hex(want[bad[0]]))
        bad = np.flatnonzero((cp_of != want) & multi)
        assert bad.size == 0, ("utf8_cp_of", w[bad[0]].tolist(), hex(cp_of[bad[0]]), hex(want[bad[0]]))
    assert int(multi.sum()) == 64 * 256 * 144


def test_lead_nibble_is_the_definition_of_a_lead_byte(harness):
    vals = np.array([0x00, 0x7F, 0x80, 0xBF, 0xC0, 0xFF], np.uint8)
    grid = np.stack([g.ravel() for g in np.meshgrid(vals, vals, vals, vals, indexing="ij")], axis=1)
    assert grid.shape == (6 ** 4, 4)
    rnd = np.random.default_rng(0x1EAD).integers(0, 256, (10000, 4)).astype(np.uint8)
    b = np.concatenate([grid, rnd])
    want = sum((((b[:, i] & 0xC0) != 0x80).astype(np.uint32) << i) for i in range(4))
    assert all(int(want[k]) == sum(int(ref.is_lead(int(x))) << i for i, x in enumerate(b[k])) for k in range(0, b.shape[0], 7))
    assert np.array_equal(harness("n", b), want)


def test_reference_is_pythons_decoder_on_well_formed_input():
    text = np.arange(0x110000, dtype="<u4").tobytes().decode("utf-32-le", "surrogatepass")
    for prefix in range(4):
        u8 = cases.all_scalars_stream(prefix)
        back = u8.tobytes().decode("utf-8", "surrogatepass")
        assert back == "abc"[:prefix] + text
        want = np.frombuffer(back.encode("utf-32-le", "surrogatepass"), "<u4")
        cps, lead = ref.decode_per_lead(u8)
        assert np.array_equal(cps, want)
        if prefix in (0, 3):
            got, pos = ref.decode_scalar(u8.tobytes())
            assert np.array_equal(np.array(got, np.uint32), want) and np.array_equal(np.array(pos), lead)
    # 4-byte leads see every dword phase over the four prefixes
    first4 = 128 + 1920 * 2 + 63488 * 3
    assert {(first4 + p) & 3 for p in range(4)} == {0, 1, 2, 3}


def _both_references(u8, byte_off):
    """(cps, rows, total) of the numpy reference, after the scalar loop has given the same"""
    cps, row, total = ref.decode_batch(u8, byte_off)
    s_cps, s_row, s_total = ref.decode_batch_scalar(np.asarray(u8, np.uint8)[:int(byte_off[-1])].tobytes(), byte_off.tolist())
    assert s_total == total and np.array_equal(np.array(s_cps, np.uint32), cps) and np.array_equal(np.array(s_row, np.int64), row)
    return cps, row, total


def test_window_stream_through_the_scalar_reference():
    u8 = cases.window_stream()
    assert u8.size == 64 * 256 * 144 * 5
    cps, row, _ = _both_references(u8, cases.cut_every(u8.size, 7))
    # the period of 5 puts window leads on every phase of dword, chunk, wave and block
    lead_pos = np.arange(0, u8.size, 5)
    for period in (4, cases.CHUNK):
        assert np.unique(lead_pos % period).size == period
    assert np.unique(lead_pos[:5 * cases.BLOCK] % cases.WAVE_BYTES).size == cases.WAVE_BYTES
    assert np.unique(lead_pos % cases.BLOCK).size == cases.BLOCK
    # strings of 7 bytes open with continuation bytes and sequences run over string ends
    off = cases.cut_every(u8.size, 7)
    assert ((u8[off[:-1]] & 0xC0) == 0x80).sum() > 100000
    # more than two non-ASCII leads in one dword (the decoder's loop for the rest), and every sequence length cut short
    assert ((u8 >= 0xC0).reshape(-1, 4).sum(axis=1) == 3).sum() > 1000      # (four: the edge stream, no window is dword aligned with b3 >= 0xC0)
    w = cases.windows(0xC0)
    w_cps = cps[np.searchsorted(ref.decode_per_lead(u8)[1], lead_pos)]
    for k, lo, hi in ((1, 0xC0, 0xE0), (2, 0xE0, 0xF0), (3, 0xF0, 0x100)):
        sel = (w[:, 0] >= lo) & (w[:, 0] < hi)
        assert (w_cps[sel] == ref.REPLACEMENT).any() and (w_cps[sel] != ref.REPLACEMENT).any(), k


def test_edge_streams_through_the_scalar_reference_and_their_census():
    u8, off = cases.edge_stream()
    _both_references(u8, off)
    ends = cases.end_of_batch_cases()
    for data, pos in ends:
        arr = np.frombuffer(data, np.uint8)
        cps, row, total = _both_references(arr, np.array([0, len(data)], np.int64))
        assert ref.is_lead(data[pos]) and 1 <= len(data) - pos <= 4
    segs = [cases.edge_segment(s, d) for s in cases.sequences() for d in range(-4, 1)]
    phases, spans, haves = cases.census(segs + [data for data, _ in ends])
    assert phases >= {(length, ph) for length in (1, 2, 3, 4) for ph in range(4)}
    assert spans >= {(kind, front) for kind in (4, cases.CHUNK, cases.WAVE_BYTES, cases.BLOCK) for front in (1, 2, 3)}
    assert haves == {0, 1, 2, 3}
    four = [np.frombuffer(x, np.uint8).reshape(-1, 4) for x in segs]
    assert sum(int(((x >= 0xC0).sum(axis=1) == 4).sum()) for x in four) >= 5        # a dword of four non-ASCII leads
    # the end-of-batch cases alone see every class of `have` (inside a stream with filler behind it is always >= 3)
    assert cases.census([data for data, _ in ends])[2] == {0, 1, 2, 3}
    # every edge is met from every d
    assert {pos for _, pos in ends} == {E + d for E in cases.EDGES for d in range(-4, 1)}


def test_string_start_streams_through_the_scalar_reference():
    u8, off = cases.string_start_case()
    cps, row, total = _both_references(u8, off)
    assert (np.diff(off) >= 0).all() and off[0] == 0 and off[-1] == u8.size
    at = off[off < u8.size]
    for c in cases.CHARS:                    # a start at every chunk offset on every byte of chars of every length
        for j in range(len(c)):
            hit = [int(p) % 16 for p in at if p >= j and bytes(u8[p - j:p - j + len(c)]) == c]
            assert set(hit) == set(range(16)), (c, j)
    runs = np.flatnonzero(np.diff(off) == 0)
    assert runs.size >= 3 * 69 + 70 and (off == u8.size).sum() == 71
    for E in (cases.WAVE_BYTES, cases.BLOCK):
        assert {E - 1, E, E + 1} <= set(off.tolist())
    for arr, boff in cases.tiny_batches():
        _both_references(arr, boff)
    assert sorted({int(b[-1]) for _, b in cases.tiny_batches()}) == [1, 15, 16, 17]


def test_big_stream_is_above_the_scan_threshold():
    scan_small_max, block = decode_limits()
    assert block == cases.BLOCK and scan_small_max >= 1
    u8 = cases.big_stream(scan_small_max * block)
    assert u8.size > scan_small_max * block and (u8.size + block - 1) // block > scan_small_max
    assert u8.size < 2 * scan_small_max * block              # the smallest that reaches the branch, within a factor of two


def test_lone_lead_blobs_hold_no_continuation_byte():
    for n, seed in ((40, 1), (5000, 2), (300000, 3)):
        blob = cases.lone_leads_blob(n, seed)
        u8 = np.frombuffer(blob, np.uint8)
        assert len(blob) >= n and not ((u8 & 0xC0) == 0x80).any() and (u8 >= 0xC0).sum() >= 4
        cps, _, total = _both_references(u8, np.array([0, u8.size], np.int64)) if n <= 5000 else ref.decode_batch(u8, np.array([0, u8.size]))
        assert total == u8.size and ((cps == ref.REPLACEMENT) == (u8 >= 0x80)).all()


def test_the_gpu_modules_own_batches_through_the_scalar_reference():
    """what tests/test_gpu_utf8_decode.py puts together itself: the pointer-mode batch and the small and large route batches"""
    import test_gpu_utf8_decode as g
    from latok_amd import batch
    u8, boff, want = g._pointer_case()
    cps, row, total = _both_references(u8, boff)
    assert total == want[2] and np.array_equal(cps, want[0]) and np.array_equal(row, want[1])
    assert u8.size > 2 * cases.BLOCK and (np.diff(boff) == 0).any()
    small = g._blobs(g.SMALL_TEXTS)
    large = list(g._large_blobs())
    for blobs in (small, small[:2] + [g.SOFT] + small[2:] + [g.HARD[:6]], large, large[:1500] + [g.SOFT, g.HARD] + large[1500:],
                  large[:1500] + [g.SOFT] + large[1500:] + [b"end\xe6"]):
        _both_references(*batch.pack_utf8(blobs))
    assert sum(map(len, large)) > 262144


def _one_well_formed_string(data):
    """every lead is followed, inside the string, by exactly the continuation bytes it announces"""
    i, n = 0, len(data)
    while i < n:
        k = ref.n_cont(data[i])
        if not ref.is_lead(data[i]) or i + k > n - 1:
            return False
        if any((b & 0xC0) != 0x80 for b in data[i + 1:i + 1 + k]):
            return False
        i += 1 + k
    return True


def test_host_decoder_of_small_batches_equals_the_reference():
    """host_decode_small (route 1) takes a batch only when every string is well formed on its own, and then gives the reference's
    code points and rows; anything else is left to the device"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_host_decode_utf8
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p] * 2 + [C.c_int64] + [C.c_void_p] * 3 + [C.POINTER(C.c_int64)]

    def host(u8, off):
        cps, row, pos, n = np.zeros(u8.size + 1, np.uint32), np.zeros(off.size, np.int64), np.zeros(u8.size + 2, np.int64), C.c_int64(-1)
        rc = fn(u8.ctypes.data, off.ctypes.data, off.size - 1, cps.ctypes.data, row.ctypes.data, pos.ctypes.data, C.byref(n))
        return rc, cps[:max(n.value, 0)], row, pos[:max(n.value, 0)]

    u8 = cases.all_scalars_stream(3)
    off = np.array([0, 2, 3, 3, 1001, u8.size], np.int64)       # cuts on char starts
    rc, cps, row, pos = host(u8, off)
    w_cps, w_row, _ = ref.decode_batch(u8, off)
    assert rc == 1 and np.array_equal(cps, w_cps) and np.array_equal(row, w_row) and np.array_equal(pos, ref.decode_per_lead(u8)[1])
    # every window as a string of its own: taken exactly when the window is one well-formed string, and then with its values
    w = cases.windows(0xC0)[::29]
    taken = 0
    for win in w.tolist():
        for n in (2, 3, 4):
            data = np.array(win[:n], np.uint8)
            rc, cps, row, _ = host(data, np.array([0, n], np.int64))
            vals, _ = ref.decode_scalar(bytes(win[:n]))
            assert rc == (1 if _one_well_formed_string(win[:n]) else 0), win[:n]
            if rc == 1:
                taken += 1
                assert cps.tolist() == vals and row.tolist() == [0, len(vals)] and ref.REPLACEMENT not in vals
    assert taken > 1000
    # a sequence that its string's end cuts is not taken, although the packed stream completes it
    data = np.frombuffer(b"ab\xe6\x97\xa5cd", np.uint8)
    assert host(data, np.array([0, 4, 7], np.int64))[0] == 0 and host(data, np.array([0, 5, 7], np.int64))[0] == 1
