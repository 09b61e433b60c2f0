"""Content, reference and census for the strip / drop logic of the span and featurize kernels under rule tables that leave
whitespace INSIDE tokens.

Under the built-in tables every unmasked whitespace char is a boundary of its own (C_SPLIT has the row [SPACE]), so a kept token
has at most one leading whitespace char and no trailing one, and a dropped token is one char long: the "far" branches of the
kernels (token longer than 64 positions, whitespace runs over several words or tiles, the keep / drop decision carried across a
word or tile edge) cannot be reached.  The tables below can reach them, and the builders plant every case at chosen bit, word and
tile positions.

Three parts, none of which calls the product:
  * TABLES / whitespace lists, checked against the oracle (``validate``);
  * ``reference``: counts, span records, spans4 records and the 25 sums of a batch from the oracle's boundaries, Python's
    ``str.strip`` and the oracle's parse matrix, in chars or in UTF-8 bytes;
  * ``census``: the set of classes (names below) a batch reaches, from the reference alone, and ``REQUIRED[size][unit]``.
Content comes from ``content(table, size, unit, rg)``: a list of batches (the classes "at the end of the batch, with / without
trailing whitespace / dropped" exclude each other inside one batch, so a size is a few batches and its census their union).
"""
import random

import numpy as np

UPPER, SPACE, SYMBOL, PREV_ALPHA = 4, 5, 6, 12                      # latok_amd/core/offsets.py
_NONE = np.zeros((0, 1), np.int8)
DEFAULT_C_MASK = np.array([[7, 18, 13, -1], [11, 18, 21, 23], [8, 14, 15, -1], [9, 22, 24, 12]], np.int8)

TABLES = {
    # tokens begin at upper-case letters only: whitespace inside a token and at its end is arbitrary
    "UPPER_ONLY": (np.array([[UPPER]], np.int8), _NONE, _NONE),
    # ... and at a whitespace char behind a letter: arbitrary leading whitespace, whitespace-only tokens of any length
    "AFTER_ALPHA": (np.array([[UPPER, -1], [SPACE, PREV_ALPHA]], np.int8), _NONE, _NONE),
    # whitespace on both sides of the text between two symbols
    "SYMBOL_ONLY": (np.array([[SYMBOL]], np.int8), _NONE, _NONE),
    # a live C_MASK (the built-in one) without the [SPACE] row in C_SPLIT: blocks open and close inside padded tokens
    "MASKED": (np.array([[UPPER], [SYMBOL]], np.int8), DEFAULT_C_MASK, _NONE),
}

TILE, SMALL_CHARS = 4096, 262144      # include/latok_hip.h: LATOK_TILE_CHARS; the pinned host route's limit (latok_debug_limits)
SIZES = ("small", "mid", "large")
UNITS = ("chars", "bytes")
RANGES = ("latin1", "bmp", "full")    # PEP 393 kind 1, kind 2, any code point

WS_LATIN1 = [chr(c) for c in range(256) if chr(c).isspace()]      # space \t \n \x0b \x0c \r \x1c-\x1f \x85 \xa0
WS = {"latin1": WS_LATIN1, "bmp": WS_LATIN1 + ["\u2003", "\u3000"], "full": WS_LATIN1 + ["\u2003", "\u3000"]}
# non-space neighbours of 1, 2, 3 and 4 UTF-8 bytes: letters (a é 日 𠀀), and chars that are no letters (1 ¿ 、 🤓) for the table
# under which whitespace behind a letter is a boundary
NB_ALPHA = ["a", "\xe9", "日", "\U00020000"]
NB_OTHER = ["1", "\xbf", "、", "\U0001F913"]


def u8len(ch):
    return len(ch.encode("utf-8", "surrogatepass"))


def in_range(ch, rg):
    return ord(ch) < {"latin1": 0x100, "bmp": 0x10000, "full": 0x110000}[rg]


def validate(oracle):
    """the whitespace chars are SPACE to the oracle exactly where str.isspace() says so, and each table does what its comment says"""
    chars = sorted(set(WS["full"] + NB_ALPHA + NB_OTHER + list("aB1!. ")))
    col = oracle.gen_parse_matrix("".join(chars))[:, SPACE]
    assert [bool(c) for c in col] == [ch.isspace() for ch in chars]
    assert all(ch.isspace() for ch in WS["full"]) and {" ", "\t", "\n", "\x1c", "\x1d", "\x1e", "\x1f", "\x85", "\xa0"} <= set(WS_LATIN1)

    def nz(name, text):
        return np.nonzero(oracle.split_values_rules(text, *TABLES[name]))[0].tolist()
    assert nz("UPPER_ONLY", "ab  Cd \t eF  ") == [0, 4, 10]
    assert nz("AFTER_ALPHA", "a" + " " * 10000 + "Bcd") == [0, 1, 10001]
    t = "A" + " " * 63 + "B" + " " * 64 + "C" + " " * 127 + "D" + " " * 128 + "E"
    b = nz("AFTER_ALPHA", t)
    assert [e - a for a, e in zip(b, b[1:]) if not t[a:e].strip()] == [63, 64, 127, 128]
    assert nz("SYMBOL_ONLY", " a  ! b  c !") == [0, 4, 11]
    assert nz("MASKED", "x  #ab!c  y!z  Q") == [0, 11, 15]        # '#' opens a block up to the next space: it and the '!' inside are masked


# ---- reference -----------------------------------------------------------------------------------------------------------
def byte_positions(t):
    """byte position of every char of t (+ one entry: its byte length), from the code points"""
    cps = np.frombuffer(t.encode("utf-32-le", "surrogatepass"), "<u4")
    pos = np.zeros(cps.size + 1, np.int64)
    np.cumsum(1 + (cps >= 0x80).astype(np.int64) + (cps >= 0x800) + (cps >= 0x10000), out=pos[1:])
    assert pos[-1] == len(t.encode("utf-8", "surrogatepass"))
    return pos


class Reference:
    """what the span and featurize entry points must return for a batch, positions in `unit`, plus one row per RAW token (kept or
    dropped) for the census"""


def reference(oracle, texts, tables, unit):
    assert unit in UNITS
    r = Reference()
    n = len(texts)
    r.unit, r.n_str = unit, n
    r.bound_counts, r.counts = np.zeros(n, np.int64), np.zeros(n, np.int64)
    r.row = np.zeros(n + 1, np.int64)
    spans4, feats, toks, offsets = [], [], [], []
    for s, t in enumerate(texts):
        cum = byte_positions(t) if unit == "bytes" else None
        r.row[s + 1] = r.row[s] + (int(cum[-1]) if unit == "bytes" else len(t))
        if not t:
            continue
        vals = oracle.split_values(t) if tables is None else oracle.split_values_rules(t, *tables)
        nz = np.nonzero(vals)[0]
        ends = np.append(nz[1:], len(t))
        sums = np.add.reduceat(oracle.gen_parse_matrix(t).view(np.uint8), nz, axis=0, dtype=np.uint8).view(np.int8)   # wraps at 256
        pos = cum.tolist() if cum is not None else None
        g0 = int(r.row[s])
        r.bound_counts[s] = nz.size
        offsets.append(cum[nz] if cum is not None else nz)
        for j, (a, e) in enumerate(zip(nz.tolist(), ends.tolist())):
            raw = t[a:e]
            kept = bool(raw.strip())
            lead = len(raw) - len(raw.lstrip()) if kept else len(raw)
            trail = len(raw) - len(raw.rstrip()) if kept else 0
            c, d = a + lead, e - trail
            pa, pe, pc, pd = (pos[a], pos[e], pos[c], pos[d]) if pos else (a, e, c, d)
            if kept:
                spans4.append((pa, pe, pc, pd))
                feats.append(sums[j])
                r.counts[s] += 1
            widths = None
            if unit == "bytes" and kept:      # (width of the char in front of the trailing run, widths in that run, width behind the leading run)
                widths = (u8len(raw[-trail - 1]), frozenset(map(u8len, raw[len(raw) - trail:])) if trail else frozenset(), u8len(raw[lead]))
            toks.append((s, g0 + pa, g0 + pe, pc - pa, pe - pd, kept, e == len(t), widths))
    r.total = int(r.row[-1])
    r.spans4 = np.array(spans4, np.int64).reshape(-1, 4)
    r.spans = np.ascontiguousarray(r.spans4[:, 2:])
    r.feats = np.array(feats, np.int8).reshape(-1, 25)
    r.offsets = np.concatenate(offsets).astype(np.int64) if offsets else np.zeros(0, np.int64)   # boundaries, relative to their string
    r.tokens = toks
    r.last_nonempty = max((s for s, t in enumerate(texts) if t), default=-1)
    r.empty = [not t for t in texts]
    return r


def compare(got, r, dtype, feats, what):
    """(counts, records[, sums]) of a span (feats False) or featurize call against the reference: exactly and in full"""
    counts, items = got[0], got[1]
    want = r.spans4 if feats else r.spans
    assert counts.dtype == dtype and items.dtype == dtype, (what, counts.dtype, items.dtype)
    assert counts.shape == r.counts.shape and np.array_equal(counts, r.counts), (what, "counts", _first_diff(counts, r.counts))
    items = items.reshape(-1, want.shape[1])
    assert items.shape == want.shape, (what, "item total", items.shape, want.shape)
    assert np.array_equal(items, want), (what, "records", _first_diff(items, want))
    if feats:
        assert got[2].dtype == np.int8 and got[2].shape == r.feats.shape and np.array_equal(got[2], r.feats), \
            (what, "sums", _first_diff(got[2], r.feats))


def _first_diff(a, b):
    """(index, returned, expected) of the first row that differs"""
    n = min(len(a), len(b))
    bad = np.nonzero(np.atleast_2d((a[:n] != b[:n]).T).any(axis=0))[0]
    return (int(bad[0]), a[bad[0]].tolist(), b[bad[0]].tolist()) if bad.size else ("lengths", len(a), len(b))


# ---- census --------------------------------------------------------------------------------------------------------------
def _bucket(v):
    return "0" if v == 0 else "1" if v == 1 else "2-63" if v < 64 else "64-127" if v < 128 else "128+"


def census(oracle, texts, tables, unit, ref=None):
    """the classes a batch reaches; positions are global positions of the packed batch in `unit` (the kernels' words and tiles)"""
    r = ref if ref is not None else reference(oracle, texts, tables, unit)
    got = set()
    n_tiles = (r.total + TILE - 1) // TILE
    bounds_in, kept_in = np.zeros(n_tiles + 1, np.int64), np.zeros(n_tiles + 1, np.int64)
    for s, p, e, lead, trail, kept, last, widths in r.tokens:
        bounds_in[p // TILE] += 1
        if kept:
            kept_in[p // TILE] += 1
            bit, wb, d = p % 64, p - p % 64, e - p
            got.add("start:" + ("0" if bit == 0 else "63" if bit == 63 else "1-62"))
            far = "fast" if d <= 63 else "next" if e < wb + 128 else "beyond"
            got.add("end:" + far)
            if d >= TILE:
                got.add("end:4096+")
            if d >= 2 * TILE:
                got.add("end:2tiles")
            got.add("lead:" + _bucket(lead))
            got.add("trail:" + _bucket(trail))
            if lead >= TILE:
                got.add("lead:4096+")
            if trail >= TILE:
                got.add("trail:4096+")
            if lead >= 64 and trail >= 64:
                got.add("lead+trail:64+")
            how = ":trail" if trail else ":clean"
            if e % 64 == 0:
                got.add("rawend:word" + how)
            if e % TILE == 0:
                got.add("rawend:tile" + how)
            if last and s < r.last_nonempty:
                got.add("rawend:string" + how)
            if e == r.total:
                got.add("rawend:batch" + how)
            if (e - trail) % 64 == 0:
                got.add("stripend:word")
            if (p + lead) // TILE > p // TILE:
                got.add("tile:first_kept_from_earlier")
            # the corners of the kernels' far branches themselves
            if far == "next" and p + lead >= wb + 64:
                got.add("far:next:owner_word_all_space")
            if far == "next" and e - trail <= wb + 64:
                got.add("far:next:next_word_all_space")
            if far == "beyond" and p + lead >= wb + 128:
                got.add("far:beyond:lead_past_next_word")
            if far == "beyond" and trail >= 128:
                got.add("far:beyond:trail_over_words")
            if widths:
                w_front, run, w_behind = widths
                if run == {2}:
                    got.add("bytes:trail2:behind%d" % w_front)
                if run == {3}:
                    got.add("bytes:trail3:behind%d" % w_front)
                if lead:
                    got.add("bytes:lead:before%d" % w_behind)
        else:
            d = e - p
            got.add("drop:" + ("1" if d == 1 else "2-63" if d < 64 else "64-4095" if d < TILE else "4096+"))
            if d >= 2 * TILE:
                got.add("drop:2tiles")
            if last:
                got.add("drop:last_of_string")
                if s + 1 < r.n_str and r.empty[s + 1]:
                    got.add("drop:then_empty_strings")
            if e == r.total:
                got.add("drop:last_of_batch")
            if p % 64 == 63:
                got.add("drop:bit63")
    if np.any((bounds_in[:n_tiles] > 0) & (kept_in[:n_tiles] == 0)):
        got.add("tile:boundaries_no_kept")
    return got


_KEPT = ["start:0", "start:1-62", "start:63", "end:fast", "end:next", "end:beyond"] + \
        [k + b for k in ("lead:", "trail:") for b in ("0", "1", "2-63", "64-127", "128+")] + \
        ["lead+trail:64+", "stripend:word"] + \
        ["rawend:%s:%s" % (w, h) for w in ("word", "tile", "string", "batch") for h in ("trail", "clean")] + \
        ["far:next:owner_word_all_space", "far:next:next_word_all_space", "far:beyond:lead_past_next_word", "far:beyond:trail_over_words"]
_DROP = ["drop:1", "drop:2-63", "drop:64-4095", "drop:last_of_string", "drop:last_of_batch", "drop:then_empty_strings", "drop:bit63",
         "tile:boundaries_no_kept"]
# what needs more than one tile: the one-launch path holds at most TILE positions, so `small` cannot reach these
_MULTI_TILE = ["end:4096+", "end:2tiles", "lead:4096+", "trail:4096+", "drop:4096+", "drop:2tiles", "tile:first_kept_from_earlier"]
_BYTES = ["bytes:%s%d" % (k, w) for k in ("trail2:behind", "trail3:behind", "lead:before") for w in (1, 2, 3, 4)]
REQUIRED = {size: {"chars": frozenset(_KEPT + _DROP + (_MULTI_TILE if size != "small" else [])),
                   "bytes": frozenset(_KEPT + _DROP + _BYTES + (_MULTI_TILE if size != "small" else []))} for size in SIZES}


# ---- content -------------------------------------------------------------------------------------------------------------
_STYLE = {   # start: a non-space char that opens a token under the table; body: ASCII chars that open none, in any context
    "UPPER_ONLY": ("B", "abc123.,;"),
    "AFTER_ALPHA": ("B", "123.,;"),
    "SYMBOL_ONLY": ("!", "abc123"),
    "MASKED": ("B", "abc123"),
}
_MASKED_PIECES = [" #ab!c ", " a@b.c ", " http://a.b/c ", " .@u "]
# target positions of the batches A, B, C of a size (D is a handful of whitespace-only strings); tokens and strings of the filler
_TARGET = {"small": (TILE, TILE, 3000), "mid": (180_000, 60_000, 20_000), "large": (2_400_000, 700_000, 300_000)}
_TOKEN_HI = {"small": 12, "mid": 40, "large": 150}
_STRING = {"small": (5, 70), "mid": (20, 3000), "large": (50, 40000)}


class _Builder:
    def __init__(self, table, size, unit, rg, seed):
        self.start, self.body_chars = _STYLE[table]
        self.table, self.size, self.unit, self.rg = table, size, unit, rg
        self.rng = random.Random(seed)
        self.ws_pool = [(c, u8len(c) if unit == "bytes" else 1) for c in WS[rg]]
        wide = [c for c in NB_ALPHA[1:] + NB_OTHER[1:] if in_range(c, rg) and (table != "SYMBOL_ONLY" or c in NB_ALPHA)]
        self.mid_pool = [(c, 1) for c in self.body_chars] * 3 + [(c, u8len(c) if unit == "bytes" else 1) for c in wide] + \
                        [(c, w) for c, w in self.ws_pool if c in " \t\xa0\u3000"]
        if table == "MASKED":
            self.mid_pool += [(p, len(p)) for p in _MASKED_PIECES]
        if table == "AFTER_ALPHA":      # a letter, whitespace, an upper-case letter: the whitespace is a token of its own, and dropped
            self.mid_pool += [("a B", 3), ("b \t\nB", 5)] * 6
        self.strings, self.cur, self.pos, self.spos = [], [], 0, 0
        self.next_cut = self.rng.randint(*_STRING[size])

    def ulen(self, s):
        return len(s.encode("utf-8")) if self.unit == "bytes" else len(s)

    def add(self, s):
        n = self.ulen(s)
        self.cur.append(s)
        self.pos += n
        self.spos += n

    def end_string(self):
        self.strings.append("".join(self.cur))
        self.cur, self.spos = [], 0

    def empty(self, k):
        assert not self.cur
        self.strings += [""] * k

    def _fit(self, pool, n):
        """a string of exactly n positions out of (text, positions) items"""
        out = []
        while n > 0:
            c, w = self.rng.choice(pool)
            if w <= n:
                out.append(c)
                n -= w
        return "".join(out)

    def ws(self, n, width=None):
        """a whitespace run of exactly n positions; width: only chars of that many UTF-8 bytes"""
        pool = [(c, w) for c, w in self.ws_pool if width is None or u8len(c) == width]
        if self.unit == "bytes" and width is not None:
            assert n % width == 0
        return self._fit(pool, n)

    def body(self, n):
        return "".join(self.rng.choice(self.body_chars) for _ in range(n - 1)) + "1"

    def kept(self, n):
        assert n >= 2
        return self.start + self.body(n - 1)

    def filler(self, n, cut=True):
        """exactly n positions of ordinary tokens: each opens with `start`, closes with '1', and has chars of every width and
        short whitespace runs in between"""
        while n > 0:
            m = min(n, self.rng.randint(2, _TOKEN_HI[self.size]))
            if n - m == 1:
                m = n
            self.add("1" if m == 1 else self.start + self._fit(self.mid_pool, m - 2) + "1")
            n -= m
            if cut and self.spos >= self.next_cut:
                self.end_string()
                self.next_cut = self.rng.randint(*_STRING[self.size])

    def pad_to(self, at, mod=64):
        d = (at - self.pos) % mod
        if d == 1:
            d += mod          # (a one-char filler would not open a token of its own)
        self.filler(d, cut=False)
        assert self.pos % mod == at

    def plant(self, text, at=None, end_on=None, mod=64, new_string=False):
        """text at global position `at` (mod `mod`), or so that it ENDS at `end_on`; new_string: as the head of a string"""
        if end_on is not None:
            at = (end_on - self.ulen(text)) % mod
        if at is not None:
            self.pad_to(at, mod)
        if new_string and self.cur:
            self.end_string()
        assert new_string or not text[0].isspace()
        self.add(text)


def _g_far(b):
    """start bits; raw ends in the next word and beyond it, with the corners of the kernels' far branches"""
    K, W, B = b.kept, b.ws, b.body
    for at in (0, 63, 17):
        b.plant(K(9), at=at)
    b.plant(K(74), at=30)
    b.plant(W(30) + B(40), at=40, new_string=True)       # next word; nothing but whitespace in the owner word
    b.plant(K(20) + W(60), at=10)                        # next word; nothing but whitespace there
    b.plant(K(72) + W(2), at=63)
    b.plant(K(200), at=5)
    b.plant(W(98) + B(10), at=50, new_string=True)       # the leading run passes the whole next word
    b.plant(K(10) + W(300), at=5)                        # the trailing run covers several words
    b.plant(W(70) + B(5) + W(90), new_string=True)
    b.plant(K(12), end_on=0)                             # raw end on a word edge, without / with trailing whitespace
    b.plant(K(12) + W(6), end_on=0)
    b.plant(K(12) + W(4), end_on=4)                      # stripped end on a word edge
    b.plant(K(8))
    b.end_string()                                       # raw end = string end, another string behind
    b.plant(K(8) + W(4))
    b.end_string()


def _g_runs(b):
    """leading and trailing runs of every range"""
    for n in (1, 2, 37, 63, 64, 100, 127, 128, 300):
        b.plant(b.ws(n) + b.body(6), new_string=True)
        b.plant(b.kept(6) + b.ws(n))


def _g_drop(b):
    for n in (1, 2, 40, 63, 64, 700):
        b.plant(b.ws(n) + b.kept(5), new_string=True)    # a dropped token, then a kept one
    b.plant(b.ws(9), new_string=True)
    b.end_string()                                       # dropped, last of its string
    b.plant(b.kept(4))
    b.end_string()
    b.plant(b.ws(5), new_string=True)
    b.end_string()
    b.empty(3)                                           # ... followed by empty strings
    b.plant(b.ws(7), at=63, new_string=True)             # ... starting at bit 63
    b.end_string()


def _g_bytes(b):
    """whitespace runs of 2-byte and of 3-byte chars behind, and any run in front of, a char of each width"""
    behind = NB_OTHER if b.table == "AFTER_ALPHA" else NB_ALPHA
    for nb_t, nb_l in zip(behind, NB_ALPHA):
        if in_range(nb_t, b.rg):
            b.plant(b.start + nb_t + b.ws(6 if b.unit == "bytes" else 3, 2))
            if b.rg != "latin1":
                b.plant(b.start + nb_t + b.ws(6 if b.unit == "bytes" else 2, 3))
        if in_range(nb_l, b.rg):
            b.plant(b.ws(5) + nb_l + b.body(3), new_string=True)
    b.plant(b.kept(3))


def _g_tiles(b):
    """what needs several tiles"""
    K, W, B = b.kept, b.ws, b.body
    b.plant(K(5000), at=3)
    b.plant(K(9000), at=20)
    b.plant(W(5000) + B(6), new_string=True)
    b.plant(K(6) + W(5000))
    for n in (4096, 5000, 9000):
        b.plant(W(n) + K(5), new_string=True)
    b.plant(K(12), end_on=0, mod=TILE)                   # raw end on a tile edge
    b.plant(K(12) + W(5), end_on=0, mod=TILE)
    b.pad_to(0, TILE)                                    # a tile with boundaries and no kept token
    b.end_string()
    for _ in range(4):
        b.add(W(1024))
        b.end_string()
    b.plant(W(200) + B(6), at=4000, mod=TILE, new_string=True)   # the next tile's first kept token begins here, in whitespace


def _finish(b, target, tail, cut=True):
    """filler up to `target` positions, the batch ending with `tail`"""
    room = target - b.pos - b.ulen(tail)
    assert room >= 0 and room != 1, (b.table, b.size, b.unit, b.rg, room)
    b.filler(room, cut)
    b.add(tail)
    b.end_string()
    assert b.pos == target
    return b.strings


def content(table, size, unit, rg="full"):
    """[A, B, C, D]: A ends with a kept token without trailing whitespace, B with one that has some, C with a dropped token and
    empty strings behind it, D holds whitespace-only strings.  Deterministic: the seed is the arguments."""
    assert unit == "chars" or rg == "full"
    ta, tb, tc = _TARGET[size]
    out = []
    for i, (target, groups) in enumerate(((ta, (_g_far,)), (tb, (_g_runs,)), (tc, (_g_drop, _g_bytes)))):
        b = _Builder(table, size, unit, rg, "%s/%s/%s/%s/%d" % (table, size, unit, rg, i))
        if size != "small":
            b.filler(target // 4)
            groups = (_g_far, _g_runs, _g_drop, _g_bytes, _g_tiles) if i == 0 else groups
        for g in groups:
            g(b)
        if i == 2:
            if size != "small":
                b.filler(max(0, target - b.pos - 64))
            if b.cur:
                b.end_string()
            b.add(b.ws(11))
            b.end_string()
            b.empty(2)
            assert size != "small" or b.pos <= TILE
            out.append(b.strings)
        else:
            out.append(_finish(b, target, b.kept(7) + (b.ws(6) if i == 1 else "")))
    b = _Builder(table, size, unit, rg, "D")
    out.append([b.ws(3), b.ws(70), "", b.ws(1), b.ws(200)])
    return out
