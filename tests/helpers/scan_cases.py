"""Inputs and expectations for the two device-wide exclusive scans of int64 counts (k_scan_chained of compact_kernels.hip and
launch_exclusive_scan of aux_kernels.hip), pure numpy.  Every size comes from the limits the library reports
(latok_debug_scan_limits); the expectation is np.cumsum in int64, shifted to the exclusive form.

The patterns are seeded and identical on every run:
  sparse    counts in 0..5 with long runs of zeros (what a row scan sees: many empty rows)
  mod7      1 + (i mod 7): no two prefixes are equal
  onehot    a single 1 at a named position: the output is a step, so an included or a skipped predecessor is off by exactly one
  wide      2^33 + small at scattered positions, so that sums cross 2^32 inside a wave, between the waves of a workgroup and between
            workgroups (the chain words, the block totals); the total stays below 2^44
  widemax   the total is exactly 2^44 - 1, the largest a published chain word holds
"""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

Limits = namedtuple("Limits", "chain_chunk lookback value_bits epoch_bits small_max scan_chunk scan_block")
ITEMS = 4          # kChainItems / kScanItems: consecutive entries one thread owns (scan_chunk = ITEMS * scan_block)
WAVE = 64
PATTERNS = ("sparse", "mod7", "wide", "widemax")
WIDE = 1 << 33


@functools.lru_cache(maxsize=1)
def limits():
    """latok_debug_scan_limits (needs no device)"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_scan_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(9, np.int64)
    assert fn(out.ctypes.data, 9) == 7
    return Limits(*(int(x) for x in out[:7]))


def tile_units():
    """kTile, entry 0 of latok_debug_limits: the device-sized chained scan takes ceil(units / kTile) entries"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(1, np.int64)
    assert fn(out.ctypes.data, 1) == 1
    return int(out[0])


# ---- lengths: each the smallest shape for the edge it names ----------------------------------------------------------------------
def chained_lengths(lim):
    c, w = lim.chain_chunk, lim.lookback
    wave_items = ITEMS * WAVE
    return [(1, "one entry"), (2, "two entries"), (WAVE - 1, "lane edge"), (WAVE, "lane edge"), (WAVE + 1, "lane edge"),
            (wave_items - 1, "wave edge"), (wave_items, "wave edge"), (wave_items + 1, "wave edge"),
            (c - 1, "one workgroup, its last thread short of one item"), (c, "one full workgroup"), (c + 1, "two workgroups"),
            (2 * c, "two full workgroups"), (2 * c + 1, "three workgroups"),
            (w * c, "ticket W - 1 is the last"), (w * c + 1, "ticket W looks at exactly W predecessors in one round"),
            ((w + 1) * c, "ticket W is the last and full"), ((w + 1) * c + 1, "the first scan with a second look-back round"),
            ((w + 2) * c + 1, "the second round holds more than one lane"),
            ((2 * w + 1) * c + 1, "three rounds"), ((2 * w + 2) * c + 3, "three rounds, two lanes in the third")]


def three_launch_lengths(lim):
    s, k, b = lim.small_max, lim.scan_chunk, lim.scan_block
    return [(1, "one entry"), (b - 1, "per = 1, the last thread empty"), (b, "per = 1, every thread one entry"),
            (b + 1, "per = 2 in k_scan_small"), (s, "the largest single-workgroup scan"), (s + 1, "the smallest three-launch scan"),
            (2 * k, "two full blocks"), (2 * k + 1, "three blocks"),
            (b * k, "one block total per thread of k_scan_totals"), (b * k + 1, "per = 2 in k_scan_totals")]


def device_sized_cases(lim):
    """(grid size n, [real sizes in entries]) of the device-sized chained scan"""
    c, w = lim.chain_chunk, lim.lookback
    n = (2 * w + 2) * c + 3
    return n, [0, 1, c, c + 1, (w + 1) * c + 1, n]


# ---- one-hot positions -----------------------------------------------------------------------------------------------------------
def onehot_positions(chunk, window=0):
    """name -> entry index of the single 1; chunk = entries per workgroup, window = workgroups per look-back round (0: none)"""
    t, wave_items = 5, ITEMS * WAVE
    pos = {"first entry": 0,
           "first item of a thread": ITEMS * t, "last item of a thread": ITEMS * t + ITEMS - 1,
           "first of a wave": wave_items, "last of a wave": 2 * wave_items - 1,
           "last of the first wave": wave_items - 1,
           "first of a workgroup chunk": chunk, "last of a workgroup chunk": 2 * chunk - 1,
           "last of the first chunk": chunk - 1}
    if window:
        # ticket `window` reads tickets window - 1 .. 0 in its first round; ticket window + 1 reads window .. 1, then ticket 0
        pos.update({"last of the first look-back window": window * chunk - 1, "first of the second window": window * chunk,
                    "first of a look-back window": chunk, "last of a look-back window": (window + 1) * chunk - 1,
                    "first behind that window": (window + 1) * chunk, "last of two windows": 2 * window * chunk - 1,
                    "first of the third window": 2 * window * chunk})
    return pos


# ---- values ----------------------------------------------------------------------------------------------------------------------
def _sparse(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 6, n, dtype=np.int64)
    run = 37
    live = np.repeat(rng.random((n + run - 1) // run) < 0.4, run)[:n]      # runs of zeros of 37 entries and more
    return v * live


def wide_positions(n, chunk, window):
    """where the 2^33 values sit: two lanes of one wave, two other waves, the next workgroups, both sides of every window edge"""
    wave_items = ITEMS * WAVE
    p = [1, ITEMS + 1, 3 * wave_items + 2, 9 * wave_items, chunk - 1, chunk + 7, 3 * chunk + 1]
    if window:
        p += [window * chunk - 2, window * chunk + 5, (window + 1) * chunk + 3, 2 * window * chunk + 1, (2 * window + 1) * chunk + 2]
    else:
        p += [17 * chunk + 3, (n // chunk) * chunk - 1, n // 2]
    p.append(n - 1)
    return sorted({x for x in p if 0 <= x < n})


def values(pattern, n, seed, chunk, window=0, value_bits=44):
    if pattern == "sparse":
        return _sparse(n, seed)
    if pattern == "mod7":
        return 1 + (np.arange(n, dtype=np.int64) + seed) % 7
    if pattern == "wide":
        v = _sparse(n, seed + 1)
        pos = np.array(wide_positions(n, chunk, window), np.int64)
        v[pos] = WIDE + 1 + np.arange(pos.size)
        return v
    if pattern == "widemax":
        v = _sparse(n, seed + 2)
        top = (1 << value_bits) - 1
        v[0] = 0
        rest = top - int(v.sum())
        if n == 1:
            v[0] = rest
        else:                      # half in the first workgroup, so that every chain word carries it, the rest in the last entry
            v[-1] = 0
            rest = top - int(v.sum())
            v[0] = rest // 2
            v[-1] = rest - rest // 2
        return v
    raise ValueError(pattern)


def onehot(n, p):
    v = np.zeros(n, np.int64)
    v[p] = 1
    return v


def expect(v, real=None):
    """(exclusive scan, total) of v[:real] in int64"""
    v = v if real is None else v[:real]
    inc = np.cumsum(v, dtype=np.int64)
    out = np.empty_like(inc)
    if v.size:
        out[0] = 0
        out[1:] = inc[:-1]
    return out, int(inc[-1]) if v.size else 0


def cases(n, seed, chunk, window=0, value_bits=44):
    """every (name, values) of length n: the four patterns and every one-hot position that fits"""
    for k, pattern in enumerate(PATTERNS):
        yield pattern, values(pattern, n, seed + 11 * k, chunk, window, value_bits)
    for name, p in onehot_positions(chunk, window).items():
        if p < n:
            yield "onehot: " + name, onehot(n, p)
