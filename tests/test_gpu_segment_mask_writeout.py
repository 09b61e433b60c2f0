"""The UTF-32 tile kernel's held segments (split_kernels.hip: run_segment, step (d)): a segment of at most kSegHoldTiles tiles
keeps its mask words in the workgroup and stores them as one contiguous run at its end.  Every case compares the mask bit for bit
with the oracle and with the same batch run with the hold switched off (the stores as they were: eight tiles at a time from the
wave's registers).  The cap comes from the library (latok_debug_tile_limits); segments are shaped with latok_debug_set_tile_plan
(segment length, most workgroups, hold on / off) and every case asserts through latok_debug_last_plan that it ran the geometry and
the path it was built for.  The plan is restored in a ``finally``.

Text: the ASCII and the mixed-Unicode corpus of latok_corpus_*, string lengths 1..300 -- tiles are not string aligned and
some need a patch from the resolve stage.  Batches stay under 1 M chars but for the two full segments of kSegHoldTiles tiles side
by side (2 x 144 tiles = 1.18 M chars)."""
import ctypes as C

import numpy as np
import pytest

from conftest import RULE_SETS, oracle_rule_bits

pytestmark = pytest.mark.gpu

TILE = 4096
SEED = 0x5E6A11
GUARD = 4                                      # guard words on each side of a mask
PATTERN = np.uint64(0xA5C3F00D5A3C0FF0)
M_BITS, M_RULES = 0, 3                         # latok::kModeBits, kModeRules (kernels.h)
PLAN_HEAD = ("mode", "small", "fixed")
PLAN_NAMES = ("n_cu_eff", "seg_tiles", "n_segs", "rounds", "grid_tiles", "grid_resolve", "fast_tail", "pf", "wpb", "nw", "one_launch",
              "n_tiles", "hold")


def _fn(name, argtypes):
    from latok_amd import _lib
    f = getattr(_lib.load(), name)
    f.restype, f.argtypes = C.c_int, argtypes
    return f


def set_tile_plan(seg_tiles=0, grid=0, hold=-1):
    from latok_amd import _lib
    _lib.check(_fn("latok_debug_set_tile_plan", [C.c_int, C.c_int, C.c_int])(seg_tiles, grid, hold))


def last_plan():
    out = np.zeros(len(PLAN_HEAD) + len(PLAN_NAMES), np.int64)
    assert _fn("latok_debug_last_plan", [C.c_void_p, C.c_int])(out.ctypes.data, out.size) == out.size
    return dict(zip(PLAN_HEAD + PLAN_NAMES, out.tolist()))


@pytest.fixture(scope="module")
def cap_tiles(gpu):
    out = np.zeros(2, np.int64)
    assert _fn("latok_debug_tile_limits", [C.c_void_p, C.c_int])(out.ctypes.data, 2) == 2
    lim = np.zeros(4, np.int64)
    assert _fn("latok_debug_limits", [C.c_void_p, C.c_int])(lim.ctypes.data, 4) == 4
    assert lim[0] == TILE and out[0] == 12 * lim[1] and 0 < out[1] < 12   # 12 rounds of kWPB tiles
    return int(out[0])


@pytest.fixture
def plan_hook(gpu):
    try:
        yield set_tile_plan
    finally:
        set_tile_plan(0, 0, -1)


_CORPUS, _WANT = {}, {}


def corpus(model, total):
    """(cps, row) of exactly `total` chars: strings of 1..300 chars of the library's corpus, the last one cut"""
    key = (model, total)
    if key not in _CORPUS:
        from latok_amd import _lib
        lib = _lib.load()
        n = total // 100 + 64
        row = np.zeros(n + 1, np.int64)
        _lib.check(lib.latok_corpus_offsets(SEED + model, 0, n, 1, 300, row.ctypes.data))
        assert row[-1] >= total
        cps = np.zeros(int(row[-1]), np.uint32)
        _lib.check(lib.latok_corpus_fill_host(SEED + model, model, 0, n, row.ctypes.data, cps.ctypes.data))
        k = int(np.searchsorted(row, total, side="left"))
        row = row[:k + 1].copy()
        row[k] = total
        assert (np.diff(row) >= 1).all()
        _CORPUS[key] = (np.ascontiguousarray(cps[:total]), row)
    return _CORPUS[key]


def want_bits(oracle, model, total):
    key = (model, total)
    if key not in _WANT:
        cps, row = corpus(model, total)
        bits = oracle.split_batch(cps, row)[1]
        bits.setflags(write=False)
        _WANT[key] = bits
    return _WANT[key]


def trim(bits, total):
    """the words of a mask with the bits past `total` in the last word cleared (they are not compared)"""
    b = np.array(bits, np.uint64)
    if total % 64:
        b[-1] &= np.uint64((1 << (total % 64)) - 1)
    return b


class Dev:
    def __init__(self):
        from latok_amd import _lib
        self.lib, self._lib, self.ptrs = _lib.load(), _lib, []

    def alloc(self, nbytes):
        p = self.lib.latok_dev_alloc(nbytes + 64)
        assert p
        self.ptrs.append(p)
        return p

    def put(self, a):
        p = self.alloc(a.nbytes)
        self._lib.check(self.lib.latok_memcpy_h2d(p, a.ctypes.data, a.nbytes))
        return p

    def mask(self, words, shift=0):
        """a guarded mask of `words` words, `shift` bytes off a 16-byte boundary: (buffer, address of word 0, words in the buffer)"""
        n = words + 2 * GUARD + 2
        p = self.alloc(n * 8)
        assert p % 16 == 0 and shift in (0, 8)
        fill = np.full(n, PATTERN, np.uint64)
        self._lib.check(self.lib.latok_memcpy_h2d(p, fill.ctypes.data, fill.nbytes))
        return p, p + GUARD * 8 + shift, n

    def get_mask(self, buf, words, n, shift=0):
        """the mask's words; the guards on both sides must hold the pattern"""
        a = np.empty(n, np.uint64)
        self._lib.check(self.lib.latok_memcpy_d2h(a.ctypes.data, buf, a.nbytes))
        lo = GUARD + shift // 8
        assert (a[:lo] == PATTERN).all(), "guard words in front of the mask"
        assert (a[lo + words:] == PATTERN).all() and a.size - lo - words >= GUARD, "guard words behind the mask"
        return a[lo:lo + words]

    def close(self):
        for p in self.ptrs:
            self.lib.latok_dev_free(p)
        self.ptrs = []


def blocking(d, dc, dr, row, words, seg, grid, hold, shift=0):
    """one blocking device-pointer call under the given plan: (mask words, what was launched)"""
    total = int(row[-1])
    buf, dm, n = d.mask(words, shift)
    set_tile_plan(seg, grid, hold)
    d._lib.check(d.lib.latok_split_mask_batch(dc, dr, row.size - 1, total, dm, d._lib.DEVICE_PTRS, None))
    p = last_plan()
    return trim(d.get_mask(buf, words, n, shift), total), p


def check_case(oracle, model, total, seg, grid, want, shift=0, expect=None, mode=M_BITS):
    """the batch under the plan (seg, grid), held and not held, against `expect` (default: the oracle) and against each other;
    `want`: entries of the launched plan (the hold flag among them)"""
    cps, row = corpus(model, total)
    words = (total + 63) // 64
    ref = trim(want_bits(oracle, model, total) if expect is None else expect, total)
    d = Dev()
    try:
        dc, dr = d.put(cps), d.put(row)
        got, p = blocking(d, dc, dr, row, words, seg, grid, -1, shift)
        assert p["mode"] == mode and p["one_launch"] == 0 and p["n_tiles"] == -(-total // TILE), p
        for k, v in want.items():
            assert p[k] == v, (k, v, p)
        old, q = blocking(d, dc, dr, row, words, seg, grid, 0, shift)
        assert q["hold"] == 0 and all(q[k] == p[k] for k in PLAN_NAMES if k != "hold"), (p, q)
        bad = np.nonzero(got != ref)[0]
        assert bad.size == 0, (f"{bad.size} words differ from the reference, first {int(bad[0])} of {words}", p)
        assert np.array_equal(old, ref), "the stores as they were"
        return p
    finally:
        d.close()


def one_segment(n_tiles, rem, cap):
    """(total, seg, want) of a batch of n_tiles tiles planned as ONE segment, the last tile holding `rem` chars"""
    total = (n_tiles - 1) * TILE + rem
    seg = max(12, n_tiles)
    return total, seg, {"seg_tiles": seg, "n_segs": 1, "grid_tiles": 1, "hold": int(seg <= cap)}


@pytest.mark.parametrize("model", [0, 1], ids=["ascii", "unicode"])
@pytest.mark.parametrize("delta", [-143, -133, -132, -131, -1, 0, 1], ids=["1", "11", "12", "13", "cap-1", "cap", "cap+1"])
def test_segment_lengths(oracle, plan_hook, cap_tiles, model, delta):
    """one segment of 1, 11, 12, 13, cap - 1 and cap tiles (held: a round and a half round of waves, one tile more and less; the
    last round of registers full) and of cap + 1 (not held)"""
    assert cap_tiles == 144
    n_tiles = cap_tiles + delta
    total, seg, want = one_segment(n_tiles, 1000 + 97 * (n_tiles % 7) + model, cap_tiles)
    assert want["hold"] == int(delta <= 0)
    check_case(oracle, model, total, seg, 0, want)


@pytest.mark.parametrize("model", [0, 1], ids=["ascii", "unicode"])
def test_two_full_segments_side_by_side(oracle, plan_hook, cap_tiles, model):
    """two segments of cap tiles in two workgroups: the boundary between two runs"""
    total = 2 * cap_tiles * TILE - 37 - model
    check_case(oracle, model, total, cap_tiles, 0, {"seg_tiles": cap_tiles, "n_segs": 2, "grid_tiles": 2, "rounds": 1, "hold": 1})


@pytest.mark.parametrize("model", [0, 1], ids=["ascii", "unicode"])
def test_one_workgroup_three_segments(oracle, plan_hook, model):
    """one workgroup walks three segments (the plan hook's grid of 1; latok_debug_set_plan_cus takes 8 CUs or more): the write-out
    runs per segment, and the next segment's tiles reuse the LDS the run was read from.  The last segment is shorter."""
    seg = 52
    total = (3 * seg - 9) * TILE - 3000 + model
    p = check_case(oracle, model, total, seg, 1, {"seg_tiles": seg, "n_segs": 3, "grid_tiles": 1, "rounds": 3, "hold": 1})
    assert p["n_tiles"] == 3 * seg - 9


@pytest.mark.parametrize("shift", [0, 8], ids=["aligned16", "aligned8"])
@pytest.mark.parametrize("r", [0, 1, 63, 64, 65, 127, 128, 4095])
def test_batch_end_and_mask_alignment(oracle, plan_hook, cap_tiles, r, shift):
    """totals of 4096 k + r: the run's last store is a pair, a single word, or ends the tile; the guard words on both sides of the
    mask stay as they were.  The same with a mask that is only 8-byte aligned (8-byte stores for the whole run)."""
    k = 13
    total = TILE * k + r
    n_tiles = -(-total // TILE)
    seg = max(12, n_tiles)
    model = (r + shift // 8) & 1
    check_case(oracle, model, total, seg, 0, {"seg_tiles": seg, "n_segs": 1, "hold": 1}, shift=shift)


def test_aligned8_two_segments(oracle, plan_hook, cap_tiles):
    """an 8-byte aligned mask with a full segment, registers and LDS rounds both in use, and a second run behind it"""
    total = (cap_tiles + 30) * TILE - 1
    check_case(oracle, 1, total, cap_tiles, 0, {"seg_tiles": cap_tiles, "n_segs": 2, "hold": 1}, shift=8)


def test_flow_sizes_straddling_the_cap(oracle, plan_hook, cap_tiles):
    """four batches through latok_flow_split_mask, two masks alternating, one segment each of cap - 1, cap, cap + 1 and cap + 6
    tiles: each equals its blocking result and the oracle.  Two masks hold the last two batches only, so the four go through
    twice, the second time in the other order."""
    from latok_amd import batch
    sizes = [cap_tiles - 1, cap_tiles, cap_tiles + 1, cap_tiles + 6]
    d = Dev()
    try:
        items = []
        for i, n_tiles in enumerate(sizes):
            total, seg, want = one_segment(n_tiles, 500 + 611 * i, cap_tiles)
            cps, row = corpus(i & 1, total)
            words = (total + 63) // 64
            dc, dr = d.put(cps), d.put(row)
            block, p = blocking(d, dc, dr, row, words, seg, 0, -1)
            assert p["hold"] == want["hold"] and p["n_segs"] == 1, p
            assert np.array_equal(block, trim(want_bits(oracle, i & 1, total), total))
            items.append((dc, dr, row, total, words, seg, want, block))
        max_words = max(it[4] for it in items)
        for order in ([0, 1, 2, 3], [2, 3, 0, 1]):
            masks = [d.mask(max_words), d.mask(max_words)]
            for j, i in enumerate(order):
                dc, dr, row, total, words, seg, want, block = items[i]
                set_tile_plan(seg, 0, -1)
                batch.flow_split_mask(dc, dr, row.size - 1, total, masks[j & 1][1])
                p = last_plan()
                assert p["hold"] == want["hold"] and p["seg_tiles"] == seg and p["one_launch"] == 0, p
            batch.flow_wait()
            for j in (2, 3):
                dc, dr, row, total, words, seg, want, block = items[order[j]]
                buf, _, n = masks[j & 1]
                got = d.get_mask(buf, max_words, n)
                # (words behind this batch's own: the guard pattern, or what the larger batch before it on this mask left)
                assert np.array_equal(trim(got[:words], total), block), (order, j)
    finally:
        d.close()


def test_rules_one_full_segment(oracle, plan_hook, cap_tiles):
    """run-time rules (kModeRules): one held segment of cap tiles"""
    from latok_amd import batch
    tables = RULE_SETS["sym_everywhere"]
    total, seg, want = one_segment(cap_tiles, 2222, cap_tiles)
    cps, row = corpus(1, total)
    texts = [cps[row[s]:row[s + 1]].astype("<u4").tobytes().decode("utf-32-le", "surrogatepass") for s in range(row.size - 1)]
    expect = oracle_rule_bits(oracle, texts, tables)
    batch.set_rules(*tables)
    try:
        check_case(oracle, 1, total, seg, 0, want, expect=expect, mode=M_RULES)
    finally:
        batch.reset_rules()


def test_flow_deep_prefetch_instantiation(oracle, plan_hook, cap_tiles):
    """a flow batch above kFastTailTiles takes the tile kernel's deep-prefetch instantiation: two held segments through it
    (257 tiles = 1.05 M chars: the smallest batch that takes it)"""
    from latok_amd import batch
    lim = np.zeros(6, np.int64)
    assert _fn("latok_debug_limits", [C.c_void_p, C.c_int])(lim.ctypes.data, 6) == 6
    n_tiles = int(lim[5]) + 1
    seg = -(-n_tiles // 2)
    assert seg <= cap_tiles
    total = n_tiles * TILE - 77
    cps, row = corpus(1, total)
    words = (total + 63) // 64
    ref = trim(want_bits(oracle, 1, total), total)
    d = Dev()
    try:
        dc, dr = d.put(cps), d.put(row)
        for hold in (-1, 0):
            buf, dm, n = d.mask(words)
            set_tile_plan(seg, 0, hold)
            batch.flow_split_mask(dc, dr, row.size - 1, total, dm)
            p = last_plan()
            batch.flow_wait()
            assert p["pf"] == 6 and p["fast_tail"] == 0 and p["n_segs"] == 2 and p["hold"] == (1 if hold else 0), p
            assert np.array_equal(trim(d.get_mask(buf, words, n), total), ref), hold
    finally:
        d.close()
