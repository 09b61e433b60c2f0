"""tests/helpers/scan_cases.py without a device: the limits hook reports its 7 values; the length lists hold every named edge for
those limits; every wide case stays below 2^44 and one case's total is 2^44 - 1 exactly; the one-hot positions sit on both ends of a
thread's items, a wave, a workgroup chunk and a look-back window; the builders are seeded and the expectation is the exclusive sum."""
import ctypes as C

import numpy as np

from helpers import scan_cases as sc


def test_limits_hook_reports_seven_values():
    from latok_amd import _lib
    lib = _lib.load()
    fn = lib.latok_debug_scan_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.full(9, -1, np.int64)
    assert fn(out.ctypes.data, 9) == 7 and (out[:7] > 0).all() and (out[7:] == -1).all()
    assert fn(out.ctypes.data, 3) == 3 and fn(None, 7) == _lib.ERR_INVALID
    lim = sc.limits()
    assert tuple(lim) == tuple(int(x) for x in out[:7])
    assert lim.lookback == sc.WAVE                                   # one predecessor per lane
    assert lim.value_bits + 2 + lim.epoch_bits == 64                 # value | flag | epoch fill one published word
    assert (1 << lim.epoch_bits) - 1 == 0x3FFFF                      # the mask latok_debug_set_scan_epoch takes (the GPU tests' epochs)
    assert lim.scan_chunk == sc.ITEMS * lim.scan_block and lim.chain_chunk % (sc.ITEMS * sc.WAVE) == 0
    assert lim.small_max >= lim.scan_block
    # the closed list of latok_debug_limits still reports kScanSmallMax as its entry 15
    old = lib.latok_debug_limits
    old.restype, old.argtypes = C.c_int, [C.c_void_p, C.c_int]
    o = np.zeros(32, np.int64)
    assert old(o.ctypes.data, 32) == 19 and int(o[15]) == lim.small_max


def test_length_lists_hold_every_named_edge():
    lim = sc.limits()
    c, w = lim.chain_chunk, lim.lookback
    chained = [n for n, _ in sc.chained_lengths(lim)]
    assert set(chained) >= {1, 2, 63, 64, 65, c - 1, c, c + 1, 2 * c, 2 * c + 1, w * c, w * c + 1, (w + 1) * c, (w + 1) * c + 1,
                            (w + 2) * c + 1, (2 * w + 1) * c + 1, (2 * w + 2) * c + 3}
    assert chained == sorted(set(chained)) and all(name for _, name in sc.chained_lengths(lim))
    blocks = lambda n: -(-n // c)                                     # noqa: E731
    rounds = lambda n: -(-(blocks(n) - 1) // w)                       # noqa: E731  look-back rounds of the last ticket
    assert rounds(w * c + 1) == 1 and rounds((w + 1) * c) == 1 and rounds((w + 1) * c + 1) == 2
    assert rounds((2 * w + 1) * c + 1) == 3 and rounds(max(chained)) == 3 and max(chained) * 8 < 5 << 20
    s, k, b = lim.small_max, lim.scan_chunk, lim.scan_block
    three = [n for n, _ in sc.three_launch_lengths(lim)]
    assert set(three) >= {1, b - 1, b, b + 1, s, s + 1, 2 * k, 2 * k + 1, b * k, b * k + 1} and three == sorted(set(three))
    per = lambda n: -(-(-(-n // k)) // b)                              # noqa: E731  block totals per thread of k_scan_totals
    assert per(b * k) == 1 and per(b * k + 1) == 2
    n, reals = sc.device_sized_cases(lim)
    assert n == max(chained) and reals == [0, 1, c, c + 1, (w + 1) * c + 1, n]


def test_wide_cases_stay_below_the_value_field():
    lim = sc.limits()
    top = 1 << lim.value_bits
    assert lim.value_bits == 44
    for lengths, chunk, window in ((sc.chained_lengths(lim), lim.chain_chunk, lim.lookback),
                                   (sc.three_launch_lengths(lim)[:8], lim.scan_chunk, 0)):
        for n, _ in lengths:
            wide = sc.values("wide", n, 5, chunk, window, lim.value_bits)
            assert wide.dtype == np.int64 and wide.min() >= 0 and 1 << 32 < int(wide.sum()) < top
            assert int(sc.values("widemax", n, 5, chunk, window, lim.value_bits).sum()) == top - 1
    # the sums cross 2^32 inside a wave, between the waves of a workgroup and between workgroups
    c, w = lim.chain_chunk, lim.lookback
    n = (2 * w + 2) * c + 3
    pos = np.array(sc.wide_positions(n, c, w))
    lane, wave, group = pos // sc.ITEMS, pos // (sc.ITEMS * sc.WAVE), pos // c
    assert wave[0] == wave[1] and lane[0] != lane[1]
    assert np.unique(wave[group == 0]).size >= 3 and np.unique(group).size >= 8
    assert {0, 1, w - 1, w, w + 1, 2 * w, 2 * w + 1} <= set(group.tolist())
    v = sc.values("wide", n, 5, c, w)
    assert (v[pos] > 1 << 33).all() and np.delete(v, pos).max() <= 5
    out, total = sc.expect(v)
    assert (out[pos[1]:] > 1 << 32).all() and total == int(v.astype(object).sum())      # no carry is lost in the reference itself


def test_onehot_positions_cover_every_edge():
    lim = sc.limits()
    c, w = lim.chain_chunk, lim.lookback
    pos = sc.onehot_positions(c, w)
    p = set(pos.values())
    assert {p_ % sc.ITEMS for p_ in (pos["first item of a thread"], pos["last item of a thread"])} == {0, sc.ITEMS - 1}
    wave = sc.ITEMS * sc.WAVE
    assert pos["first of a wave"] % wave == 0 and pos["last of a wave"] % wave == wave - 1 and 0 in p and wave - 1 in p
    assert {c - 1, c, 2 * c - 1} <= p
    assert {w * c - 1, w * c, c, (w + 1) * c - 1, (w + 1) * c} <= p                   # windows [0, W) and [1, W + 1) of tickets W, W + 1
    plain = set(sc.onehot_positions(lim.scan_chunk).values())
    assert {0, sc.ITEMS - 1 + 5 * sc.ITEMS, wave, lim.scan_chunk - 1, lim.scan_chunk, 2 * lim.scan_chunk - 1} <= plain
    assert max(p) < (2 * w + 2) * c + 3


def test_patterns_are_seeded_and_the_expectation_is_exclusive():
    lim = sc.limits()
    n = 3 * lim.chain_chunk + 5
    for pattern in sc.PATTERNS:
        a, b = (sc.values(pattern, n, 9, lim.chain_chunk, lim.lookback) for _ in range(2))
        assert a.dtype == np.int64 and a.size == n and np.array_equal(a, b)
    sparse = sc.values("sparse", n, 9, lim.chain_chunk)
    assert 0 <= sparse.min() and sparse.max() == 5 and (sparse == 0).mean() > 0.5
    zero = np.flatnonzero(np.diff(np.concatenate(([1], (sparse == 0).astype(np.int8), [1]))))
    assert (zero[1::2] - zero[::2]).max() >= 37                                          # a long run of empty rows
    mod7 = sc.values("mod7", n, 0, lim.chain_chunk)
    assert mod7[:8].tolist() == [1, 2, 3, 4, 5, 6, 7, 1] and np.unique(sc.expect(mod7)[0]).size == n
    out, total = sc.expect(np.array([3, 0, 2, 5], np.int64))
    assert out.tolist() == [0, 3, 3, 5] and total == 10
    out, total = sc.expect(np.array([3, 0, 2, 5], np.int64), real=2)
    assert out.tolist() == [0, 3] and total == 3
    out, total = sc.expect(np.array([3, 0, 2, 5], np.int64), real=0)
    assert out.size == 0 and total == 0
    step, _ = sc.expect(sc.onehot(10, 4))
    assert step.tolist() == [0] * 5 + [1] * 5
    names = [name for name, _ in sc.cases(n, 1, lim.chain_chunk, lim.lookback)]
    assert names[:4] == list(sc.PATTERNS) and len(names) == len(set(names)) and all(v.size == n for _, v in sc.cases(n, 1, lim.chain_chunk))
