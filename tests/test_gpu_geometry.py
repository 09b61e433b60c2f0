"""Every launch geometry of the tile pipeline (k_tile_index -> k_tiles_main -> k_resolve_fix, or k_one_segment) against the
reference-shaped oracle.

The plan of a batch depends on its tile count and on the CUs it is planned for (latok::plan_launch): tiles per segment
(kWPB .. kSegMax), segments per workgroup (`rounds`), the resolve stage's waves (NW = 2 / 4 / 12), the FAST_TAIL and flow
(deeper prefetch) variants of the tile kernel and the one-launch path.  On a full chip most of these need hundreds of
millions of chars, so most cases cap the plan at a few CUs (latok_debug_set_plan_cus): a smaller grid only makes each
persistent workgroup walk more segments.  Every case asserts through latok_debug_last_plan that it ran the geometry it
was built for, and the last test asserts that the file reached every required geometry.

Content is planted where the cross-tile and cross-segment carry is hardest: masked blocks that open in one segment and
close in the next, blocks that stay open for more than a whole segment, one and several pending starts entering a tile,
strings that start on a tile's first char, empty strings and one-tile strings at segment edges."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import RULE_SETS

pytestmark = pytest.mark.gpu

LIMIT_NAMES = ("kTile", "kWPB", "kNarrowWPB", "kSegMax", "kOneSegTiles", "kFastTailTiles", "kSmallChars", "kSmallStrings",
               "kCompressWaves")
PLAN_NAMES = ("n_cu_eff", "seg_tiles", "n_segs", "rounds", "grid_tiles", "grid_resolve", "fast_tail", "pf", "wpb", "nw", "one_launch",
              "n_tiles")
M_BITS, M_VALUES, M_RULES, M_BYTES, M_LATIN1, M_UCS2 = 0, 1, 3, 4, 5, 6
M_BYTES_RULES, M_LATIN1_RULES, M_UCS2_RULES, M_VALUES_RULES = 7, 8, 9, 10
THREADS = min(16, os.cpu_count() or 1)
SEEN = set()   # (form, seg_tiles, nw, rounds > 1, flow, fast_tail, one_launch, small) of every checked call


def _fn(name, argtypes):
    from latok_amd import _lib
    f = getattr(_lib.load(), name)
    f.restype, f.argtypes = C.c_int, argtypes
    return f


def limits():
    out = np.zeros(len(LIMIT_NAMES), np.int64)
    assert _fn("latok_debug_limits", [C.c_void_p, C.c_int])(out.ctypes.data, out.size) == out.size
    return dict(zip(LIMIT_NAMES, out.tolist()))


def plan(n_tiles, n_cu, in_flow, mode):
    out = np.zeros(len(PLAN_NAMES), np.int64)
    f = _fn("latok_debug_plan", [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int])
    assert f(n_tiles, n_cu, int(in_flow), mode, out.ctypes.data, out.size) == out.size
    return dict(zip(PLAN_NAMES, out.tolist()))


def last_plan():
    out = np.zeros(3 + len(PLAN_NAMES), np.int64)
    assert _fn("latok_debug_last_plan", [C.c_void_p, C.c_int])(out.ctypes.data, out.size) == out.size
    d = dict(zip(PLAN_NAMES, out[3:].tolist()))
    d.update(mode=int(out[0]), small=int(out[1]), fix_count=int(out[2]))
    return d


def set_plan_cus(n):
    from latok_amd import _lib
    _lib.check(_fn("latok_debug_set_plan_cus", [C.c_int])(n))


@pytest.fixture(scope="module")
def L(gpu):
    return limits()


@pytest.fixture(scope="module")
def device_cus(gpu):
    """the device's CU count: the largest cap latok_debug_set_plan_cus accepts"""
    return _real_cus()


@pytest.fixture
def cap():
    """cap the tile pipeline's plan at n CUs for the test; always restored"""
    def set_(n):
        set_plan_cus(n)
    try:
        yield set_
    finally:
        set_plan_cus(0)


# ---- content -------------------------------------------------------------------------------------------------------
def _arr(s):
    return np.frombuffer(s.encode("utf-32-le", "surrogatepass"), "<u4").astype(np.uint32)


POOLS = {
    "utf32": ["abc", "Hello", "camelCase", "x", "42", " ", " ", " ", "  ", "\t", ", ", ". ", "http://a.b/c", "a@b.c", ".@user",
              "#tag", "noSpacesHereAtAll_x9", "été", "日本", "\U0001f913", "á", "　", "Ⅷ", " ",
              "жд"],
    "latin1": ["abc", "Hello", "camelCase", "x", "42", " ", " ", " ", "\t", ", ", "http://a.b/c", "a@b.c", ".@user", "#tag",
               "noSpacesHere", "été", " ", "×", "ÿ¿", "µx"],
    "bmp": ["abc", "Hello", "camelCase", "x", "42", " ", " ", " ", "\t", ", ", "http://a.b/c", "a@b.c", ".@user", "#tag",
            "noSpacesHere", "été", "日本", "　", "Ⅷ", "ж", "\ud800", "￿", "á"],
    "ascii": ["abc", "Hello", "camelCase", "x", "42", " ", " ", " ", "\t", ", ", "http://a.b/c", "a@b.c", ".@user", "#tag",
              "noSpacesHere"],
}
ONE_START = _arr("http://")                     # one block start (the ':')
MULTI_START = _arr("http://ahttp://bhttp://c")   # three starts, no space between them
SPACED = _arr(" w" * 40)


def utf8_len(cps):
    return 1 + (cps >= 0x80) + (cps >= 0x800) + (cps >= 0x10000)


def fill(rng, n, pool, chunk=1 << 24):
    """n code points of random pool pieces (index arithmetic, no per-char loop; chunks keep the index arrays small)"""
    if n > chunk:
        out = np.empty(n, np.uint32)
        for a in range(0, n, chunk):
            out[a:a + chunk] = fill(rng, min(chunk, n - a), pool, chunk)
        return out
    pieces = [_arr(p) for p in POOLS[pool]]
    flat = np.concatenate(pieces)
    starts = np.cumsum([0] + [len(p) for p in pieces])[:-1]
    lens = np.array([len(p) for p in pieces], np.int64)
    k = n // int(lens.mean()) + 64
    idx = rng.integers(0, len(pieces), k)
    ln = lens[idx]
    while ln.sum() < n:
        idx = np.concatenate([idx, rng.integers(0, len(pieces), k)])
        ln = lens[idx]
    pos0 = np.cumsum(ln) - ln
    src = np.repeat(starts[idx] - pos0, ln) + np.arange(int(ln.sum()))
    return flat[src[:n]].copy()


OFFSETS = (-65, -64, -3, -2, -1, 0, 1, 2, 3, 64)


def corpus(rng, total, seg_chars, pool="utf32", n_tile_edges=300, long_block=True, ascii_before=0, want_blocked=False):
    """(cps, row_off): `total` code points of random pieces with structures planted at every segment edge (multiples of
    seg_chars) and at a sample of tile edges.  ascii_before: no multi-byte char before that position.  want_blocked: also
    return the mask of positions inside planted structures (no string boundary there, and nothing else may overwrite them)."""
    T = 4096
    cps = fill(rng, total, pool)
    if ascii_before:
        a = min(ascii_before, total)
        cps[:a] = fill(rng, a, "ascii")
    blocked = np.zeros(total + 1, bool)   # no string boundary inside a planted structure
    forced = []
    seg_edges = list(range(seg_chars, total, seg_chars)) if seg_chars else []
    tile_edges = sorted(set(rng.choice(np.arange(T, total, T), min(n_tile_edges, max(0, (total - 1) // T)), replace=False).tolist())
                        if total > T else [])
    edges = [(e, True) for e in seg_edges] + [(e, False) for e in tile_edges if e not in set(seg_edges)]

    def put(p, a):
        lo, hi = max(p, 0), min(p + len(a), total)
        if lo < hi:
            cps[lo:hi] = a[lo - p:hi - p]
            blocked[lo + 1:hi] = True
        return hi

    # A block with no closing for more than a whole segment: three starts 400 chars before the first segment edge, then no
    # space until 1.3 segments later, all in ONE string -- the pending-start queue crosses the whole second segment.
    # Planted first; no other structure and no string boundary goes inside it.
    lb_lo = lb_hi = -1
    if long_block and len(seg_edges) >= 2:
        e = seg_edges[0]
        body = np.full(int(seg_chars * 1.3), ord("q"), np.uint32)
        body[::97] = ord("/")
        block = np.concatenate([MULTI_START, body, SPACED])
        assert e - 400 + block.size + 300 < total, "the long block needs more than two segments after its start"
        lb_lo, lb_hi = e - 400, put(e - 400, block)
    for i, (e, is_seg) in enumerate(edges):
        d = OFFSETS[i % len(OFFSETS)]
        kind = (i // len(OFFSETS) + i) % 6
        p = e + d
        if p < 200 or p > total - 200 or (lb_lo - 200 <= e <= lb_hi + T + 200):
            continue
        if kind == 0:     # one pending start entering the tile: a masked block opens before p and closes after it
            put(p - len(ONE_START) - 5, np.concatenate([ONE_START, np.full(45, ord("x"), np.uint32), SPACED[:6]]))
        elif kind == 1:   # several pending starts entering the tile: recomputed by the resolve stage
            put(p - len(MULTI_START), np.concatenate([MULTI_START, np.full(3, ord("y"), np.uint32), SPACED]))
        elif kind == 2:   # a string that ends on an open block at the tile edge, and one that starts there with an e-mail
            put(e - 40, np.concatenate([_arr(" http://"), np.full(32, ord("x"), np.uint32)]))
            put(e, np.concatenate([_arr("a@"), np.full(60, ord("m"), np.uint32), _arr(".org ")]))
            blocked[e] = False
            forced.append(e)
        elif kind == 3:   # empty strings at the edge, and (at segment edges) a one-tile string behind them
            forced += [e, e]
            if is_seg and e + T < total:
                forced.append(e + T)
                blocked[e + 1:e + T] = True
        elif kind == 4:   # the tile's tail block turns out cleared: a start just before the edge, its closing space right after
            put(p - 12, np.concatenate([_arr(".@user"), np.full(6 + 3, ord("z"), np.uint32), _arr(" ")]))
        else:             # #tag and .@user starts right at the edge
            put(p - 2, _arr(" #t.@u "))
    # strings: random lengths (mean ~1500) and the planted boundaries, never inside a planted structure
    k = max(1, total // 1500)
    cuts = np.unique(rng.integers(1, total, k)) if total > 1 else np.zeros(0, np.int64)
    cuts = np.sort(np.concatenate([cuts, np.array(forced, np.int64)]))
    cuts = cuts[~blocked[cuts]]
    row = np.concatenate([[0], cuts, [total]]).astype(np.int64)
    if lb_lo >= 0:   # the string that holds the long block's starts reaches past the end of the segment after them
        s = int(np.searchsorted(row, lb_lo + 1, side="right")) - 1
        assert row[s] <= lb_lo and row[s + 1] > seg_edges[1], (row[s], row[s + 1], seg_edges[:2])
    return (cps, row, blocked) if want_blocked else (cps, row)


# ---- oracle ----------------------------------------------------------------------------------------------------------
def _chunks(row, parts):
    """string ranges [s0, s1) of about equal chars"""
    n = row.size - 1
    want = np.linspace(0, row[-1], parts + 1)
    cut = np.unique(np.concatenate([[0], np.searchsorted(row, want[1:-1]), [n]]))
    return list(zip(cut[:-1], cut[1:]))


def oracle_values(oracle, cps, row):
    """split values of the whole batch from the oracle, split at string boundaries over a thread pool"""
    out = np.zeros(int(row[-1]), np.uint8)

    def run(r):
        s0, s1 = r
        a, b = int(row[s0]), int(row[s1])
        if b > a:
            out[a:b] = oracle.split_batch(cps[a:b], row[s0:s1 + 1] - a, want_bits=False)[0]
    with ThreadPoolExecutor(THREADS) as ex:
        list(ex.map(run, _chunks(row, 4 * THREADS)))
    return out


def oracle_values_rules(oracle, cps, row, tables):
    out = np.zeros(int(row[-1]), np.uint8)

    def run(r):
        for s in range(*r):
            a, b = int(row[s]), int(row[s + 1])
            if b > a:
                t = cps[a:b].astype("<u4").tobytes().decode("utf-32-le", "surrogatepass")
                out[a:b] = oracle.split_values_rules(t, *tables).astype(np.uint8)
    with ThreadPoolExecutor(THREADS) as ex:
        list(ex.map(run, _chunks(row, 4 * THREADS)))
    return out


def pack_bits(flags):
    n = flags.size
    return np.packbits(np.concatenate([flags, np.zeros((-n) % 64, bool)]), bitorder="little").view(np.uint64)


def expect_offsets(vals, row):
    """(counts, string-relative offsets) from per-char split values"""
    nz = np.nonzero(vals)[0]
    sid = np.searchsorted(row, nz, side="right") - 1
    counts = np.bincount(sid, minlength=row.size - 1)
    return counts, nz - row[sid]


_SPACE_CACHE = {}


def space_flags(oracle, cps):
    """the oracle's SPACE column (feature 5) for every char, through a table of the distinct code points"""
    u, inv = np.unique(cps, return_inverse=True)
    key = u.tobytes()
    if key not in _SPACE_CACHE:
        t = u.astype("<u4").tobytes().decode("utf-32-le", "surrogatepass")
        _SPACE_CACHE[key] = oracle.gen_parse_matrix(t)[:, 5] != 0
    return _SPACE_CACHE[key][inv]


def expect_spans(vals, row, space):
    """token spans (default_tokenizer.py:149-158 on the device's terms): between consecutive boundaries (and the string
    end), SPACE chars stripped from both ends, empty tokens dropped; string relative"""
    n = vals.size
    nz = np.nonzero(vals)[0]
    sid = np.searchsorted(row, nz, side="right") - 1
    nxt = np.minimum(np.append(nz[1:], n), row[sid + 1])      # a token ends at the next boundary or its string's end
    last_bnd = np.ones(nz.size, bool)
    last_bnd[:-1] = sid[1:] != sid[:-1]
    nxt = np.where(last_bnd, row[sid + 1], nxt)
    ns = np.nonzero(~space)[0]
    first = ns[np.minimum(np.searchsorted(ns, nz), ns.size - 1)] if ns.size else np.full(nz.size, n)
    lastp = ns[np.maximum(np.searchsorted(ns, nxt) - 1, 0)] if ns.size else np.full(nz.size, -1)
    keep = (first < nxt) & (first >= nz) if ns.size else np.zeros(nz.size, bool)
    st, en, s = first[keep], lastp[keep] + 1, sid[keep]
    counts = np.bincount(s, minlength=row.size - 1)
    return counts, np.stack([st - row[s], en - row[s]], 1)


def to_utf8(cps, row):
    """UTF-8 bytes (surrogatepass) + byte offsets + byte position of every char, with numpy"""
    ln = utf8_len(cps)
    bpos = np.zeros(cps.size + 1, np.int64)
    np.cumsum(ln, out=bpos[1:])
    out = np.zeros(int(bpos[-1]), np.uint8)
    p = bpos[:-1]
    c = cps.astype(np.int64)
    for n, lead in ((1, 0), (2, 0xC0), (3, 0xE0), (4, 0xF0)):
        m = ln == n
        cc, pp = c[m], p[m]
        if n == 1:
            out[pp] = cc
            continue
        out[pp] = lead | (cc >> (6 * (n - 1)))
        for k in range(1, n):
            out[pp + k] = 0x80 | ((cc >> (6 * (n - 1 - k))) & 63)
    return out, bpos[row], bpos


# ---- the library's calls on one batch ---------------------------------------------------------------------------------
class Dev:
    """device copies of host arrays, freed in close()"""

    def __init__(self):
        from latok_amd import _lib
        self.lib = _lib.ensure_init()
        self.ptrs = []

    def put(self, a, extra=64):
        from latok_amd import _lib
        p = self.lib.latok_dev_alloc(a.nbytes + extra)
        assert p
        self.ptrs.append(p)
        if a.nbytes:
            _lib.check(self.lib.latok_memcpy_h2d(p, a.ctypes.data, a.nbytes))
        return p

    def empty(self, nbytes):
        p = self.lib.latok_dev_alloc(nbytes + 64)
        assert p
        self.ptrs.append(p)
        return p

    def get(self, p, n, dtype):
        from latok_amd import _lib
        a = np.empty(n, dtype)
        if a.nbytes:
            _lib.check(self.lib.latok_memcpy_d2h(a.ctypes.data, p, a.nbytes))
        return a

    def close(self):
        for p in self.ptrs:
            self.lib.latok_dev_free(p)
        self.ptrs = []


def seen(form, p, flow=False):
    SEEN.add((form, p["seg_tiles"], p["nw"], p["rounds"] > 1, flow, p["fast_tail"], p["one_launch"], p["small"]))


def check_plan(form, mode, n_units, want, flow=False):
    """the last call launched what the plan for its size says, in `mode`, and (want) the geometry the case was built for"""
    got = last_plan()
    assert got["mode"] == mode, (form, got)
    assert got["n_tiles"] == -(-n_units // 4096), (form, got)
    ref = plan(got["n_tiles"], want.get("n_cu", got["n_cu_eff"]) if not flow else want["n_cu"], flow, mode)
    for k in PLAN_NAMES:
        assert got[k] == ref[k], (form, k, got, ref)
    for k, v in want.items():
        if k != "n_cu":
            assert got[k] == v, (form, k, v, got)
    seen(form, got, flow)
    return got


def first_diff(a, b):
    bad = np.nonzero(a != b)[0]
    return f"{bad.size} diffs, first at {int(bad[0])}" if bad.size else "equal"


def check_utf32(oracle, cps, row, vals, want, rules=None, device=True, spans=True):
    """UTF-32 forms of one batch: mask (host, device), values, offsets int64 / int32, token spans"""
    from latok_amd import _lib, batch
    bits = pack_bits(vals != 0)
    m = M_RULES if rules else M_BITS
    got = batch.split_mask_batch(cps, row)
    assert np.array_equal(got, bits), ("mask", first_diff(got, bits))
    p = check_plan("utf32_mask_rules" if rules else "utf32_mask", m, cps.size, want)
    gv = batch.split_values_batch(cps, row)
    assert np.array_equal(gv, vals), ("values", first_diff(gv, vals))
    # (the values modes have no one-launch or FAST_TAIL variant and resolve with 12 waves)
    vwant = {k: v for k, v in want.items() if k in ("n_cu", "seg_tiles", "rounds", "n_segs")}
    check_plan("values_rules" if rules else "values", M_VALUES_RULES if rules else M_VALUES, cps.size,
               {**vwant, "nw": 12} if not p["one_launch"] else {k: v for k, v in vwant.items() if k == "n_cu"})
    if rules:
        return p
    counts, offs = expect_offsets(vals, row)
    for dt in (np.int64, np.int32):
        c, o = batch.split_offsets_csr(cps, row, dtype=dt)
        assert np.array_equal(c, counts) and np.array_equal(o, offs), ("offsets", dt)
    if spans:
        sc, ss = expect_spans(vals, row, space_flags(oracle, cps))
        for dt in (np.int64, np.int32):
            c, s = batch.token_spans_csr(cps, row, dtype=dt)
            assert np.array_equal(c, sc) and np.array_equal(s.reshape(-1, 2), ss), ("spans", dt)
    if device:
        d = Dev()
        try:
            dc, dr, dm = d.put(cps), d.put(row), d.empty(bits.nbytes)
            lib = d.lib
            _lib.check(lib.latok_split_mask_batch(dc, dr, row.size - 1, int(row[-1]), dm, _lib.DEVICE_PTRS, None))
            assert np.array_equal(d.get(dm, bits.size, np.uint64), bits), "device mask"
            check_plan("utf32_mask_dev", m, cps.size, want)
        finally:
            d.close()
    return p


def check_bytes(oracle, cps, row, vals, want, rules=False, cp_utf8=True):
    """byte-space forms of the same text: mask / offsets / spans at byte positions; code-point UTF-8 (mask_utf8_via_bytes)"""
    from latok_amd import batch
    u8, boff, bpos = to_utf8(cps, row)
    flags = np.zeros(u8.size, bool)
    flags[bpos[:-1][vals != 0]] = True
    bits = pack_bits(flags)
    got = batch.split_mask_utf8_bytes_csr(u8, boff)
    assert np.array_equal(got, bits), ("byte mask", first_diff(got, bits))
    p = check_plan("bytes_mask_rules" if rules else "bytes_mask", M_BYTES_RULES if rules else M_BYTES, u8.size, want)
    if rules:
        return p
    counts, offs = expect_offsets(vals, row)
    boffs = bpos[offs + np.repeat(row[:-1], counts)] - np.repeat(boff[:-1], counts)
    for dt in (np.int64, np.int32):
        c, o = batch.split_offsets_utf8_bytes_csr(u8, boff, dtype=dt)
        assert np.array_equal(c, counts) and np.array_equal(o, boffs), ("byte offsets", dt)
    if cp_utf8:
        gm, grow = batch.split_mask_utf8_csr(u8, boff)
        assert np.array_equal(grow, row) and np.array_equal(gm, pack_bits(vals != 0)), "code-point UTF-8 mask"
        check_plan("cp_utf8_mask", M_BYTES, u8.size, want)
        for dt in (np.int64, np.int32):
            c, o = batch.split_offsets_utf8_csr(u8, boff, dtype=dt)
            assert np.array_equal(c, counts) and np.array_equal(o, offs), ("code-point UTF-8 offsets", dt)
    return p


def check_kind(units, row, vals, kind, want, rules=False):
    from latok_amd import batch
    got = batch.split_mask_kind_csr(units, row)
    bits = pack_bits(vals != 0)
    assert np.array_equal(got, bits), ("kind", kind, first_diff(got, bits))
    mode = {(1, False): M_LATIN1, (2, False): M_UCS2, (1, True): M_LATIN1_RULES, (2, True): M_UCS2_RULES}[(kind, rules)]
    p = check_plan(f"kind{kind}" + ("_rules" if rules else ""), mode, units.size, want)
    if not rules:
        counts, offs = expect_offsets(vals, row)
        c, o = batch.split_offsets_kind_csr(units, row)
        assert np.array_equal(c, counts) and np.array_equal(o, offs), ("kind offsets", kind)
    return p


# ---- geometry -----------------------------------------------------------------------------------------------------------
CAP = 8
SEG_TARGETS = (12, 128, 129, 256, 257, 767, 768)
REMS = (4096, 1, 63, 64, 4095)      # total % 4096 in {0, 1, 63, 64, 4095}


def tiles_for_seg(seg, n_cu):
    """a tile count whose plan on n_cu CUs (one round) has segments of exactly `seg` tiles"""
    return seg * n_cu


def geometry_cases(L):
    """(name, n_tiles, want) for the capped blocking runs"""
    wpb, seg_max = L["kWPB"], L["kSegMax"]
    cases = [(f"seg{s}", tiles_for_seg(s, CAP), {"seg_tiles": s, "rounds": 1}) for s in SEG_TARGETS]
    # rounds = 2: 16 segments of s tiles, the last one short by one tile (s > kSegMax / 2 so that one round cannot hold them)
    s2 = seg_max // 2 + 16
    cases.append(("rounds2_short1", 2 * CAP * s2 - 1, {"seg_tiles": s2, "rounds": 2}))
    # a last segment of one tile (plan_segments only makes one at the kWPB floor, where one round holds every segment)
    cases.append(("last_seg_1tile", wpb * (CAP - 1) + 1, {"seg_tiles": wpb, "n_segs": CAP}))
    return cases


def _rem(i):
    return REMS[i % len(REMS)]


@pytest.mark.parametrize("idx", range(9))
def test_capped_blocking_geometry(L, oracle, cap, idx):
    """Capped at 8 CUs: segments of 12 ... 768 tiles (both edges of NW = 2, 4 and 12), two segments per workgroup, a last
    segment short by one tile and one of a single tile; UTF-32 mask (host and device), values, offsets, spans, run-time
    rules, byte space with and without rules, code-point UTF-8, and PEP 393 kinds 1 and 2, all against the oracle."""
    name, n_tiles, want = geometry_cases(L)[idx]
    cap(CAP)
    rng = np.random.default_rng(1000 + idx)
    total = (n_tiles - 1) * L["kTile"] + _rem(idx)
    p0 = plan(n_tiles, CAP, False, M_BITS)
    for k, v in want.items():
        assert p0[k] == v, (name, k, p0)
    seg_chars = p0["seg_tiles"] * L["kTile"]
    want = {**want, "n_cu": CAP}
    cps, row = corpus(rng, total, seg_chars)
    vals = oracle_values(oracle, cps, row)
    p = check_utf32(oracle, cps, row, vals, want)
    if p["nw"] != 12:
        assert p["nw"] * 64 >= p["seg_tiles"] > (p["nw"] // 2) * 64 or p["nw"] == 2
    got = last_plan()   # (the device mask call was the last one; several pending starts enter tiles: recomputed)
    assert got["fix_count"] > 0, got
    # byte space: a text whose UTF-8 length has the same tile count (multi-byte chars are rare in it)
    del vals
    bcps, brow = _byte_text(rng, total, seg_chars, ascii_before=(seg_chars * (CAP + 1) if p0["rounds"] > 1 else 0))
    bvals = oracle_values(oracle, bcps, brow)
    check_bytes(oracle, bcps, brow, bvals, want)
    # run-time rules: every start (maximum pressure on the queue) and every context column, UTF-32 mask + values, byte space
    if idx in (2, 4, 6):   # (the rule oracle runs string by string in Python: segments of 129, 257 and 768 tiles only)
        from latok_amd import batch
        for rname in ("all_starts", "all_columns"):
            tables = RULE_SETS[rname]
            batch.set_rules(*tables)
            try:
                rv = oracle_values_rules(oracle, cps, row, tables)
                check_utf32(oracle, cps, row, rv, {k: v for k, v in want.items() if k != "nw"}, rules=tables)
                brv = oracle_values_rules(oracle, bcps, brow, tables)
                check_bytes(oracle, bcps, brow, brv, {k: v for k, v in want.items() if k != "nw"}, rules=True)
            finally:
                batch.reset_rules()
    # PEP 393 kinds 1 and 2 (16-wave narrow kernels) on their own Latin-1 / BMP corpora
    for kind, pool, dt in ((1, "latin1", np.uint8), (2, "bmp", np.uint16)):
        kcps, krow = corpus(rng, total, seg_chars, pool=pool)
        kvals = oracle_values(oracle, kcps, krow)
        check_kind(kcps.astype(dt), krow, kvals, kind, want)


def _byte_text(rng, total_bytes, seg_bytes, ascii_before=0):
    """code points whose UTF-8 encoding is exactly total_bytes long; planted structures at byte-segment edges"""
    cps, row, blocked = corpus(rng, total_bytes, seg_bytes, pool="ascii", want_blocked=True)
    # a few multi-byte chars (2, 3 and 4 bytes) replace ASCII runs of the same byte length, never inside a planted structure
    # (blocked[i]: i lies inside one; a run [p, p + n) touches a structure iff blocked[p .. p + n] has a hit)
    pos = np.sort(rng.choice(np.arange(max(ascii_before, 8), max(total_bytes - 8, ascii_before + 9)), min(2000, total_bytes // 64),
                             replace=False)) if total_bytes > ascii_before + 64 else np.zeros(0, np.int64)
    cps_out = cps.copy()
    repl = np.array([0x00E9, 0x65E5, 0x1F913], np.uint32)
    mb_len = np.array([2, 3, 4])
    drop = np.zeros(cps.size, bool)
    last = -8
    for i, p in enumerate(pos.tolist()):
        k = i % 3
        n = int(mb_len[k])
        if (p - last < 8 or p + n > cps.size or blocked[p:p + n + 1].any() or ((row > p) & (row < p + n)).any()
                or (cps[p:p + n] >= 0x80).any()):
            continue
        cps_out[p] = repl[k]
        drop[p + 1:p + n] = True
        last = p
    # remove the chars the multi-byte ones replaced; row offsets move with them
    shift = np.concatenate([[0], np.cumsum(drop)])
    new_row = row - shift[row]
    out = cps_out[~drop]
    assert int(utf8_len(out).sum()) == total_bytes
    return out, new_row


def test_byte_space_second_segment_first_multibyte(L, oracle, cap):
    """rounds = 2: a workgroup's first segment is pure ASCII, the batch's first multi-byte char lies in its second segment
    (the lazy class table of byte space, tables_ensure_bytes, in a workgroup that has already run a segment)."""
    cap(CAP)
    rng = np.random.default_rng(77)
    s2 = L["kSegMax"] // 2 + 16
    n_tiles = 2 * CAP * s2 - 3
    total = (n_tiles - 1) * L["kTile"] + 777
    p0 = plan(n_tiles, CAP, False, M_BYTES)
    assert p0["rounds"] == 2 and p0["grid_tiles"] == CAP
    seg_bytes = p0["seg_tiles"] * L["kTile"]
    first_mb = seg_bytes * (CAP + 1) + 123456          # segment CAP + 1: workgroup 1's second segment
    cps, row = _byte_text(rng, total, seg_bytes, ascii_before=first_mb)
    bpos = np.concatenate([[0], np.cumsum(utf8_len(cps))])
    first = int(bpos[np.argmax(cps >= 0x80)])
    assert (cps >= 0x80).any() and (CAP + 1) * seg_bytes <= first < (CAP + 2) * seg_bytes   # in workgroup 1's second segment
    vals = oracle_values(oracle, cps, row)
    check_bytes(oracle, cps, row, vals, {"n_cu": CAP, "rounds": 2, "seg_tiles": p0["seg_tiles"]}, cp_utf8=False)


def _flow_run(oracle, form, units, row, kind, vals_bits, n_cu, want):
    from latok_amd import batch
    d = Dev()
    try:
        du, dr, dm = d.put(units), d.put(row), d.empty(vals_bits.nbytes)
        n_str, total = row.size - 1, int(row[-1])
        if form == "flow_utf32":
            batch.flow_split_mask(du, dr, n_str, total, dm)
            mode = M_BITS
        elif form == "flow_bytes":
            batch.flow_split_mask_utf8_bytes(du, dr, n_str, total, dm)
            mode = M_BYTES
        else:
            batch.flow_split_mask_kind(du, kind, dr, n_str, total, dm)
            mode = M_LATIN1 if kind == 1 else M_UCS2
        batch.flow_wait()
        got = d.get(dm, vals_bits.size, np.uint64)
        assert np.array_equal(got, vals_bits), (form, first_diff(got, vals_bits))
        return check_plan(form, mode, total, {"n_cu": n_cu, **want}, flow=True)
    finally:
        d.close()


def flow_edge_tiles(edge, n_cu, mode):
    """tile counts whose FLOW plans on n_cu CUs have the longest segments <= edge and the shortest > edge.  (The flow picks,
    among CU shares of 7/8, 13/16 and 3/4, one whose segments end in a well-filled round, so not every length occurs: on 64
    CUs no flow plan has segments of exactly 256 or 257 tiles.)"""
    below, above = {}, {}
    for t in range(edge * (n_cu * 3 // 4) - 8 * n_cu, (edge + 24) * n_cu):
        st = plan(t, n_cu, True, mode)["seg_tiles"]
        (below if st <= edge else above).setdefault(st, t)
    lo, hi = max(below), min(above)
    assert edge - lo < 12 and hi - edge <= 12, (edge, lo, hi)
    return below[lo], above[hi]


@pytest.mark.parametrize("which", ["cap64", "device"])
def test_flow_geometry(L, oracle, cap, device_cus, which):
    """The flow (latok_flow_split_mask / _kind / _utf8_bytes): batches above kFastTailTiles take the flow variant of the
    tile kernel (deeper prefetch) and a CU share of 7/8, 13/16 or 3/4.  Capped at 64 CUs (the share needs 64 or more):
    segments on both sides of the NW = 2 / 4 and 4 / 12 edges (the nearest lengths the flow's plans take) for UTF-32 and byte
    space, and
    NW = 2 and 4 for PEP 393 kinds 1 and 2; at the device's own count, NW = 2.  Against the oracle.
    (Not run through the flow: 768-tile segments and two rounds per workgroup, which need 43 000+ tiles (176 M chars) per
    batch at a cap of 64; they are checked blocking, capped at 8 CUs, and the 280 M-char batch of test_uncapped_full_parity
    goes through the flow with segments of more than 256 tiles.)"""
    n_cu = 64 if which == "cap64" else device_cus
    cap(n_cu)
    rng = np.random.default_rng(5 if which == "cap64" else 6)
    if which == "cap64":
        a, b = flow_edge_tiles(128, n_cu, M_BITS)
        c, d = flow_edge_tiles(256, n_cu, M_BITS)
        sizes = [(3000, True), (a, False), (b, True), (c, False), (d, False)]
    else:
        sizes = [(3000, True)]
    for i, (n_tiles, kinds) in enumerate(sizes):
        total = (n_tiles - 1) * L["kTile"] + _rem(i + 2)
        p = plan(n_tiles, n_cu, True, M_BITS)
        assert p["pf"] == 6 and p["fast_tail"] == 0 and p["n_cu_eff"] < n_cu
        seg_chars = p["seg_tiles"] * L["kTile"]
        cps, row = corpus(rng, total, seg_chars)
        vals = oracle_values(oracle, cps, row)
        _flow_run(oracle, "flow_utf32", cps, row, 4, pack_bits(vals != 0), n_cu, {"seg_tiles": p["seg_tiles"]})
        del vals, cps, row
        bcps, brow = _byte_text(rng, total, seg_chars)
        bvals = oracle_values(oracle, bcps, brow)
        u8, boff, bpos = to_utf8(bcps, brow)
        flags = np.zeros(u8.size, bool)
        flags[bpos[:-1][bvals != 0]] = True
        _flow_run(oracle, "flow_bytes", u8, boff, 0, pack_bits(flags), n_cu, {"seg_tiles": p["seg_tiles"]})
        del u8, bvals, flags, bcps, brow
        if not kinds:   # (the kinds' other NW edges are checked blocking, capped at 8 CUs)
            continue
        for kind, pool, dt in ((1, "latin1", np.uint8), (2, "bmp", np.uint16)):
            kcps, krow = corpus(rng, total, plan(n_tiles, n_cu, True, M_LATIN1 if kind == 1 else M_UCS2)["seg_tiles"] * L["kTile"],
                                pool=pool)
            kvals = oracle_values(oracle, kcps, krow)
            _flow_run(oracle, f"flow_kind{kind}", kcps.astype(dt), krow, kind, pack_bits(kvals != 0), n_cu, {})


def test_thresholds_from_limits(L, oracle, cap):
    """One char / one string on each side of every threshold, taken from latok_debug_limits: the pinned small path
    (kSmallChars, kSmallStrings), the one-launch path (kOneSegTiles tiles, host and device pointers) and FAST_TAIL
    (kFastTailTiles tiles, blocking and in the flow: 256 tiles FAST_TAIL, 257 the flow variant)."""
    T, sc, ss, one, fast = L["kTile"], L["kSmallChars"], L["kSmallStrings"], L["kOneSegTiles"], L["kFastTailTiles"]
    rng = np.random.default_rng(31)
    cases = [(sc, 100, True), (sc + 1, 100, False), (50000, ss, True), (50000, ss + 1, False), (sc, ss, True),
             (sc + 1, ss, False), (sc, ss + 1, False)]
    for total, n_str, small in cases:
        cps, _ = corpus(rng, total, 0, n_tile_edges=20, long_block=False)
        cuts = np.sort(rng.choice(np.arange(1, total), n_str - 1, replace=False))
        row = np.concatenate([[0], cuts, [total]]).astype(np.int64)
        vals = oracle_values(oracle, cps, row)
        check_utf32(oracle, cps, row, vals, {}, device=False)
        got = last_plan()   # the spans call went through the compaction path; re-run the mask to read the split path
        from latok_amd import batch
        assert np.array_equal(batch.split_mask_batch(cps, row), pack_bits(vals != 0))
        got = last_plan()
        assert got["small"] == int(small), (total, n_str, got)
        seen("small_path", got)
    for n_tiles, one_l, ft in ((one, 1, 0), (one + 1, 0, 1), (fast, 0, 1), (fast + 1, 0, 0)):
        for edge in (0, 1):   # the last tile full, or holding one char
            total = n_tiles * T if edge == 0 else (n_tiles - 1) * T + 1
            cps, row = corpus(rng, total, 0, n_tile_edges=40, long_block=False)
            vals = oracle_values(oracle, cps, row)
            p = check_utf32(oracle, cps, row, vals, {"one_launch": one_l, "fast_tail": ft}, spans=False)
            seen("threshold", p)
    # the flow at kFastTailTiles: FAST_TAIL at 256 tiles, the flow's prefetch variant at 257
    for n_tiles, ft, pf in ((fast, 1, 2), (fast + 1, 0, 6)):
        total = n_tiles * T - 5
        cps, row = corpus(rng, total, 0, n_tile_edges=40, long_block=False)
        vals = oracle_values(oracle, cps, row)
        got = _flow_run(oracle, "flow_utf32", cps, row, 4, pack_bits(vals != 0), _real_cus(), {"fast_tail": ft, "pf": pf})
        SEEN.add(("flow_fast_tail_edge", ft, pf))
        assert got["fast_tail"] == ft


def _real_cus():
    """the device's CU count (latok_device_props)"""
    from latok_amd import _lib
    lib = _lib.ensure_init()
    n = C.c_int(0)
    _lib.check(lib.latok_device_props(C.byref(n), None, None, 0))
    assert n.value >= 8
    return n.value


def test_lead_compress_dense_shortcut(L, oracle):
    """k_lead_compress copies the words of a workgroup whose tiles are all lead bytes when its first code point opens an
    output word (compact_kernels.hip, the dense shortcut).  A mixed UTF-8 prefix of exactly one compress workgroup's bytes
    with a lead count that is (case 0) or is not (case 1) a multiple of 64, then ASCII for more than two workgroups, ending
    at a length that is not a multiple of 64: code-point mask, offsets and spans (int32 / int64) against the UTF-32 path
    and the oracle."""
    from latok_amd import batch
    T, W = L["kTile"], L["kCompressWaves"]
    wg = W * T
    rng = np.random.default_rng(8)
    for case in (0, 1):
        # the prefix: 2-byte chars and ASCII, wg bytes, leads = wg - n2 (n2 two-byte chars)
        n2 = 1024 if case == 0 else 1000 + 3      # wg - n2 a multiple of 64 or not
        assert ((wg - n2) % 64 == 0) == (case == 0)
        pre = fill(rng, wg - 2 * n2, "ascii")
        mb = np.full(n2, 0x00E9, np.uint32)
        pos = np.sort(rng.choice(np.arange(wg - n2), n2, replace=False))
        merged = np.empty(wg - n2, np.uint32)
        is_mb = np.zeros(wg - n2, bool)
        is_mb[pos] = True
        merged[is_mb] = mb
        merged[~is_mb] = pre
        tail = fill(rng, 4 * wg + 3 * T + 37, "ascii")   # (the whole batch above kSmallChars: the device path)
        cps = np.concatenate([merged, tail])
        assert int(utf8_len(cps[:wg - n2]).sum()) == wg and (cps.size + n2) % 64 != 0
        cuts = np.sort(rng.choice(np.arange(1, cps.size), 300, replace=False))
        row = np.concatenate([[0], cuts, [cps.size]]).astype(np.int64)
        vals = oracle_values(oracle, cps, row)
        u8, boff, _ = to_utf8(cps, row)
        assert u8.size > L["kSmallChars"]      # the device path (mask_utf8_via_bytes), not the host decoder
        gm, grow = batch.split_mask_utf8_csr(u8, boff)
        assert np.array_equal(grow, row) and np.array_equal(gm, pack_bits(vals != 0)), case
        assert np.array_equal(gm, batch.split_mask_batch(cps, row))
        counts, offs = expect_offsets(vals, row)
        sc, ss = expect_spans(vals, row, space_flags(oracle, cps))
        for dt in (np.int64, np.int32):
            c, o = batch.split_offsets_utf8_csr(u8, boff, dtype=dt)
            assert np.array_equal(c, counts) and np.array_equal(o, offs), (case, dt)
            c, s = batch.token_spans_utf8_csr(u8, boff, dtype=dt)
            assert np.array_equal(c, sc) and np.array_equal(s.reshape(-1, 2), ss), (case, dt)
            w = batch.token_spans_csr(cps, row, dtype=dt)
            assert np.array_equal(s, w[1]), (case, dt)
        SEEN.add(("dense_shortcut", case))


@pytest.mark.parametrize("size", ["mid", "large"])
def test_uncapped_full_parity(L, oracle, device_cus, size):
    """At the device's own CU count, no sampling: one batch with segments of (128, 256] tiles (~150 M chars), one with more
    than 256 (~280 M chars), the latter blocking and through the flow.  Host memory stays under ~3 GB; device buffers are
    freed in finally."""
    from latok_amd import batch
    T = L["kTile"]
    n_tiles = device_cus * (144 if size == "mid" else 267)
    p = plan(n_tiles, device_cus, False, M_BITS)
    assert (128 < p["seg_tiles"] <= 256) if size == "mid" else p["seg_tiles"] > 256
    rng = np.random.default_rng(90 if size == "mid" else 91)
    total = (n_tiles - 1) * T + 63
    cps, row = corpus(rng, total, p["seg_tiles"] * T, n_tile_edges=2000)
    bits = pack_bits(oracle_values(oracle, cps, row) != 0)
    got = batch.split_mask_batch(cps, row)
    assert np.array_equal(got, bits), first_diff(got, bits)
    del got
    check_plan("utf32_mask_full", M_BITS, total, {"n_cu": device_cus, "seg_tiles": p["seg_tiles"]})
    if size == "large":
        pf = plan(n_tiles, device_cus, True, M_BITS)
        got = _flow_run(oracle, "flow_utf32", cps, row, 4, bits, device_cus, {"seg_tiles": pf["seg_tiles"]})
        assert got["seg_tiles"] > 256


def _module_case_count():
    """test cases this module defines besides test_zz_coverage (parametrized ones once per parameter set)"""
    n = 0
    for name, f in globals().items():
        if name.startswith("test_") and name != "test_zz_coverage" and callable(f):
            k = 1
            for m in getattr(f, "pytestmark", []):
                if m.name == "parametrize":
                    k *= len(m.args[1])
            n += k
    return n


def test_zz_coverage(request):
    """The file reached every required geometry (runs last): a case that silently stops reaching its geometry fails here.
    Only meaningful when every case of the module was selected (a -k subset skips it)."""
    here = [it for it in request.session.items if it.module is not None and it.module.__name__ == __name__
            and it.originalname != "test_zz_coverage"]
    if len(here) < _module_case_count():
        pytest.skip("coverage is asserted over the whole module; only a subset of it was selected")
    calls = [t for t in SEEN if len(t) == 8]      # (form, seg_tiles, nw, rounds > 1, flow, fast_tail, one_launch, small)
    segs = {(t[0], t[1]) for t in calls}
    for form in ("utf32_mask", "utf32_mask_dev", "values", "bytes_mask", "cp_utf8_mask", "kind1", "kind2"):
        for s in SEG_TARGETS:
            assert (form, s) in segs, (form, s)
    for form in ("utf32_mask_rules", "values_rules", "bytes_mask_rules"):
        for s in (129, 257, 768):
            assert (form, s) in segs, (form, s)
    nws = {(t[0], t[2]) for t in calls}
    for form in ("flow_utf32", "flow_bytes"):   # both sides of both NW edges
        for lo, hi in ((0, 128), (129, 140), (245, 256), (257, 268)):
            assert any(f == form and lo <= st <= hi for f, st in segs), (form, lo, hi)
    for form in ("utf32_mask", "bytes_mask", "kind1", "kind2", "flow_utf32", "flow_bytes", "flow_kind1", "flow_kind2"):
        for nw in ((2, 4) if form in ("flow_kind1", "flow_kind2") else (2, 4, 12)):
            assert (form, nw) in nws, (form, nw)
    rounds2 = {t[0] for t in calls if t[3]}
    assert {"utf32_mask", "bytes_mask", "cp_utf8_mask", "kind1", "kind2", "values"} <= rounds2
    assert any(t[0] == "utf32_mask" and t[6] == 1 for t in calls)          # one launch
    assert any(t[0] == "threshold" and t[5] == 1 for t in calls)           # FAST_TAIL
    assert {t[7] for t in calls if t[0] == "small_path"} == {0, 1}
    assert ("flow_fast_tail_edge", 1, 2) in SEEN and ("flow_fast_tail_edge", 0, 6) in SEEN
    assert ("dense_shortcut", 0) in SEEN and ("dense_shortcut", 1) in SEEN
    assert any(t[0] == "utf32_mask_full" and 128 < t[1] <= 256 for t in calls)
    assert any(t[0] == "utf32_mask_full" and t[1] > 256 for t in calls)
    assert any(t[0] == "flow_utf32" and t[1] > 256 and t[4] for t in calls)
