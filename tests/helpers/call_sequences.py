"""Plans, batches, references and the driver of the call-sequence tests (tests/test_call_sequences_host.py,
tests/test_gpu_call_sequences.py): every entry-point family after every other on ONE context.

Nothing here imports the library under test.  A FAMILY is any object with

  name                  a string
  call(batch, occ)      runs the entry point on ``batch`` (``occ`` = how often this family ran before in the plan: the output width is int64
                        on even and int32 on odd occurrences) and returns {array name: array}; or a callable that returns that dict when
                        it is asked later (an asynchronous call: the driver asks only after the NEXT step has been enqueued)
  expect(batch)         {array name: array or Approx}: the reference, computed once per (family, batch, width) unless ``stateful`` is set
                        (then it is asked after every call: the family's expectation depends on what it has seen)

and the driver holds every step of a plan to its expectation -- it skips nothing and filters nothing; the first difference raises a
SequenceError that names the step, the predecessor and its batch, the family, the batch, the width, the array and the index.

  pair_cover(n)         a cyclic sequence of n * n + 1 indices in which every ordered pair (a, b), a == b included, is adjacent once
  pair_cover_touching(n, new)   the same for the pairs that have a member of ``new`` in them, and no other pair
  after_each(r, f)      every refusing step followed once by every family
  rotation(plan, ..)    the batch of every step: contents alternate DENSE, SPARSE, the sparse batch never longer than the dense one before it
  build_batches(..)     the batches E, S, S600, SN, M, M5, L in both contents, fixed seeds, sized by the library's thresholds (passed in)
  Reference             the plain restatement of every byte-space / code-point result over one batch: boundaries and feature columns
                        come from the oracle, everything else is numpy and collections over them"""
import collections
import random

import numpy as np

DENSE, SPARSE = "DENSE", "SPARSE"
SIZE_NAMES = ("E", "S", "S600", "SN", "M", "M5", "L")
CUT = b"\xe6\x97"                      # U+65E5 without its last byte: the cut 3-byte sequence that ends one string of every batch
WIDTHS = ("int64", "int32")


# ---- plans ---------------------------------------------------------------------------------------------------------------------------
def pair_cover(n):
    """A de Bruijn sequence of order 2 over n symbols, closed: an Euler circuit of the complete directed graph with loops, walked by
    Hierholzer's rule with every vertex's exits in an order fixed by a seeded shuffle.  n * n + 1 elements, n * n adjacent pairs, all
    different.  (The lexicographic circuit 0, 0 1, 0 2, .. would do for the pairs, but its period ties a family's position to the
    parity of the step: a family would meet one content, one width and few sizes.)"""
    if n < 1:
        raise ValueError("n must be >= 1")
    rng = random.Random(0xC0FFEE + n)
    exits = {a: rng.sample(range(n), n) for a in range(n)}
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if exits[v]:
            stack.append(exits[v].pop())
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


def pair_cover_touching(n, new):
    """The part of pair_cover(n) that has a member of ``new`` in it, closed: every ordered pair (a, b) of range(n) with a in new or b in
    new adjacent exactly once, a == b for a new a included, and no pair of two old indices.  In that graph a new vertex has n exits and
    n entries, an old one len(new) of each, and every vertex reaches a new one in one step: an Euler circuit exists.  Walked by the
    same rule as pair_cover, exits in an order fixed by a seeded shuffle, from the lowest new index.  n * n - (n - len(new)) ** 2 pairs,
    one element more."""
    new = sorted(set(new))
    if n < 1 or not new or new[0] < 0 or new[-1] >= n:
        raise ValueError("new must be a non-empty subset of range(n)")
    is_new = set(new)
    rng = random.Random(0xC0FFEE + n)
    exits = {}
    for a in range(n):
        to = list(range(n)) if a in is_new else new
        exits[a] = rng.sample(to, len(to))
    stack, circuit = [new[0]], []
    while stack:
        v = stack[-1]
        if exits[v]:
            stack.append(exits[v].pop())
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


def pairs_of(plan):
    return list(zip(plan[:-1], plan[1:]))


def after_each(refusers, families):
    """[r, f, r, f', ...]: every index of ``refusers`` directly in front of every index of ``families``, once"""
    plan = []
    for r in refusers:
        for f in families:
            plan += [r, f]
    return plan


# (size of the dense step, size of the sparse step behind it): the sparse one is never longer
CYCLE = (("M5", "M5"), ("M", "S600"), ("M", "M"), ("S600", "S"), ("M5", "M"), ("S", "E"), ("SN", "S600"), ("SN", "S"), ("M5", "SN"))
L_EVERY, L_FIRST = 8, 3


def rotation(plan, uses_l):
    """[(size name, content)] per step: step k is DENSE for even k and SPARSE for odd k; each pair of steps takes the pair of CYCLE that
    a fixed multiplicative hash of its number picks (the plan's own period would otherwise pin a family to few sizes).  A family that
    takes L (uses_l[family]) gets it at its occurrences 3, 11, 19, ...: one step in eight of its own, fewer of the plan's."""
    out, occ = [], collections.Counter()
    for k, f in enumerate(plan):
        size = CYCLE[((((k // 2) * 2654435761) & 0xFFFFFFFF) >> 13) % len(CYCLE)][k % 2]
        if uses_l[f] and occ[f] % L_EVERY == L_FIRST:
            size = "L"
        occ[f] += 1
        out.append((size, SPARSE if k % 2 else DENSE))
    return out


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
class SequenceError(AssertionError):
    def __init__(self, step, pred, pred_batch, family, batch, width, array, index, got, want):
        self.step, self.pred, self.pred_batch, self.family, self.batch = step, pred, pred_batch, family, batch
        self.width, self.array, self.index, self.got, self.want = width, array, index, got, want
        super().__init__("step %d: %s on %s (%s) after %s on %s: array %r differs first at %r: got %r, want %r" %
                         (step, family, batch, width, pred, pred_batch, array, index, got, want))


class Approx:
    """a float expectation: |got - want| <= bound * |want| element by element, exact zero where want is zero, no NaN or infinity"""

    def __init__(self, want, bound):
        self.want = np.asarray(want, np.float64)
        self.bound = np.broadcast_to(np.asarray(bound, np.float64), self.want.shape)

    def first_difference(self, got):
        got = np.asarray(got)
        if got.shape != self.want.shape:
            return "shape", got.shape, self.want.shape
        g = got.astype(np.float64)
        bad = ~np.isfinite(g) | (np.abs(g - self.want) > self.bound * np.abs(self.want))
        if not bad.any():
            return None
        i = int(np.flatnonzero(bad)[0])
        return i, float(g.flat[i]), float(self.want.flat[i])


def first_difference(got, want):
    """None, or (index, got value, want value) of the first element in which two arrays differ; shapes count"""
    if isinstance(want, Approx):
        return want.first_difference(got)
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shape", got.shape, want.shape
    if got.dtype.kind in "iub" and want.dtype.kind in "iub" and got.dtype != want.dtype:
        wide = np.uint64 if np.uint64 in (got.dtype, want.dtype) else np.int64
        got, want = got.astype(wide), want.astype(wide)
    bad = got != want
    if not np.any(bad):
        return None
    i = np.argwhere(bad)[0]
    i = int(i[0]) if i.size == 1 else tuple(int(x) for x in i)
    return i, got[i].item() if hasattr(got[i], "item") else got[i], want[i].item() if hasattr(want[i], "item") else want[i]


def _key(batch):
    return getattr(batch, "key", batch)


def run(plan, families, sizes, on_step=None, errors=None):
    """Run ``plan`` (indices into ``families``) with the batch ``sizes[k]`` at step k.  Returns the number of steps executed and judged,
    which is len(plan) or the call raised.  on_step(k, family, batch, occ) is told of every step after its call.  ``errors``: a list that
    takes every SequenceError instead of the first one being raised -- for a diagnosis that wants all of them; the tests pass none."""
    if len(sizes) != len(plan):
        raise ValueError("one batch per step")
    cache, occ, pending, judged = {}, collections.Counter(), None, 0

    def judge(k, width, got, want):
        fam, batch = families[plan[k]], sizes[k]
        pred = (families[plan[k - 1]].name, _key(sizes[k - 1])) if k else (None, None)
        names = sorted(set(got) | set(want))
        for name in names:
            if name not in got or name not in want:
                d = ("presence", name in got, name in want)
            else:
                d = first_difference(got[name], want[name])
            if d is not None:
                err = SequenceError(k, pred[0], pred[1], fam.name, _key(batch), width, name, *d)
                if errors is None:
                    raise err
                errors.append(err)

    def want_of(k, width):
        fam, batch = families[plan[k]], sizes[k]
        if getattr(fam, "stateful", False):
            return fam.expect(batch)
        ck = (fam.name, _key(batch), width)
        if ck not in cache:
            cache[ck] = fam.expect(batch)
        return cache[ck]

    for k, f in enumerate(plan):
        fam, batch = families[f], sizes[k]
        o = occ[f]
        occ[f] += 1
        width = WIDTHS[o % 2]
        got = fam.call(batch, o)
        want = want_of(k, width)
        if pending is not None:                       # the step before was asynchronous: this one is enqueued behind it, now read it
            pk, pw, pgot, pwant = pending
            pending = None
            judge(pk, pw, pgot(), pwant)
            judged += 1
        if callable(got):
            pending = (k, width, got, want)
        else:
            judge(k, width, got, want)
            judged += 1
        if on_step is not None:
            on_step(k, fam, batch, o)
    if pending is not None:
        pk, pw, pgot, pwant = pending
        judge(pk, pw, pgot(), pwant)
        judged += 1
    return judged


# ---- text ----------------------------------------------------------------------------------------------------------------------------
ASCII_LETTERS = "abcdefghijklmnopqrstuvwxyz"
WIDE_LETTERS = ["\xe9", "ж", "日", "あ", "\U00010437"]          # 2, 2, 3, 3 and 4 bytes
SYMBOLS = [".", ",", ";", "!"]
SEPARATORS = [" ", "\t", " ", ".", " ", ",", "\t", ";", " ", "!"]              # each one char; the symbols are tokens of their own


def _long_word(i):
    """8 .. 29 lower-case letters, a function of i alone"""
    r = random.Random(7000 + i)
    return "".join(r.choice(ASCII_LETTERS[:20]) for _ in range(8 + (i * 7) % 22))


LONG_WORDS = [_long_word(i) for i in range(48)]
LONG_IN_VOCAB = 36                                                             # LONG_WORDS[36:] are out of vocabulary
VOCAB_WORDS = [w.encode("utf-8") for w in list(ASCII_LETTERS) + WIDE_LETTERS + SYMBOLS + LONG_WORDS[:LONG_IN_VOCAB] + ["́"]] + \
              [b"a b", b"c d e", (LONG_WORDS[0] + " " + LONG_WORDS[1]).encode()]             # words that hold the n-gram separator
WP_PREFIX = b"##"
WP_WORDS = [b"[PAD]", b"[UNK]", b"[CLS]", b"[SEP]"] + [w.encode("utf-8") for w in list(ASCII_LETTERS) + WIDE_LETTERS + SYMBOLS] + \
           [w.encode() for w in LONG_WORDS[:6]] + [(a + b).encode() for a in ASCII_LETTERS[:20:2] for b in ASCII_LETTERS[:20:3]] + \
           [b"##" + c.encode() for c in ASCII_LETTERS[:20] if c not in "gq"] + [b"##" + (a + b).encode() for a in "abcd" for b in "efgh"]


def _dense_text(rng, n_chars):
    out = []
    for _ in range(max(n_chars // 2, 1)):
        out.append(rng.choice(WIDE_LETTERS) if rng.random() < 0.15 else rng.choice(ASCII_LETTERS))
        out.append(rng.choice(SEPARATORS))
    return "".join(out[:max(n_chars, 1)]).rstrip(" \t") or "a"


def _sparse_text(rng, n_chars):
    out, n = [], 0
    while n < n_chars:
        w = rng.choice(LONG_WORDS)
        out.append(w)
        n += len(w) + 1
    return " ".join(out)[:n_chars].rstrip(" ") or "a"


_FILL = {DENSE: b"a b\tc.d e,f g;h i ", SPARSE: (" ".join(LONG_WORDS[30:40]) + " ").encode()}


def _filler(content, n, phase=0):
    pat = _FILL[content]
    reps = (n + phase) // len(pat) + 2
    return (pat * reps)[phase:phase + n]


class Batch:
    """One batch in every input form: ``u8`` / ``boff`` (UTF-8, as the byte-space and code-point calls take it), ``cps`` / ``row`` (its
    decoded code points: the UTF-32 form; the cut sequence is U+FFFD), ``k1`` (every code point above 0xFF replaced by U+00E9, as
    uint8) and ``k2`` (every code point above 0xFFFF replaced by U+3042, as uint16), both with ``row``."""

    def __init__(self, size, content, blobs):
        self.size, self.content, self.key, self.blobs = size, content, "%s/%s" % (size, content), blobs
        self.boff = np.zeros(len(blobs) + 1, np.int64)
        np.cumsum([len(b) for b in blobs], out=self.boff[1:])
        raw = b"".join(blobs)
        self.u8 = np.frombuffer(raw, np.uint8).copy() if raw else np.zeros(0, np.uint8)
        self.n_str, self.total_bytes = len(blobs), len(raw)
        from helpers import utf8_ref
        self.cps, self.row, self.total_chars = utf8_ref.decode_batch(self.u8, self.boff)
        self.cps = np.ascontiguousarray(self.cps, np.uint32)
        self.lead = np.flatnonzero((self.u8 & 0xC0) != 0x80)
        self.k1 = np.where(self.cps > 0xFF, 0xE9, self.cps).astype(np.uint8)
        self.k2 = np.where(self.cps > 0xFFFF, 0x3042, self.cps).astype(np.uint16)
        self._ref = {}

    def __repr__(self):
        return "Batch(%s: %d strings, %d bytes, %d chars)" % (self.key, self.n_str, self.total_bytes, self.total_chars)


def _fit(blobs, at, content, total):
    """make the byte total exact by resizing the ASCII filler string blobs[at]"""
    rest = sum(len(b) for i, b in enumerate(blobs) if i != at)
    if total - rest < 8:
        raise ValueError("no room for the filler string: %d of %d" % (rest, total))
    blobs[at] = _filler(content, total - rest)
    return blobs


def _with_edges(blobs, at, content, tile):
    """put a token across every tile edge that falls inside the ASCII filler string blobs[at]: a 3-byte letter (DENSE) or a run of
    letters (SPARSE) from one byte in front of the edge"""
    start = sum(len(b) for b in blobs[:at])
    s = bytearray(blobs[at])
    edge = (start // tile + 1) * tile
    while edge + 4 < start + len(s):
        p = edge - start
        if p >= 4:
            if content == DENSE:
                s[p - 2:p + 3] = b" \xe6\x97\xa5 "
            else:
                s[p - 3:p + 3] = b"zzzzzz"
        edge += tile
    blobs[at] = bytes(s)
    return blobs


def _strings(rng, content, n, lo, hi):
    gen = _dense_text if content == DENSE else _sparse_text
    return [gen(rng, rng.randint(lo, hi)).encode("utf-8") for _ in range(n)]


def _extras(content):
    """what a SPARSE batch of several strings also holds: a run of empty strings and one row of marks only"""
    return [b"", b"", b"", b"", "́́́".encode("utf-8"), b""] if content == SPARSE else []


def build_batch(size, content, tile, small_chars, small_strings):
    rng = random.Random("%s/%s" % (size, content))
    if size == "E":
        return Batch(size, content, [b"", b"", b""])
    if size == "S":                                    # one string of 37 bytes that ends in the cut sequence
        return Batch(size, content, [_filler(content, 35) + CUT])
    if size == "SN":                                   # one string more than the pinned small route takes, in less than a tile: S600 and empty strings
        blobs = build_batch("S600", content, tile, small_chars, small_strings).blobs
        return Batch(size, content, blobs + [b""] * (small_strings + 1 - len(blobs)))
    if size == "S600":                                 # 600 strings, 3001 bytes
        if content == DENSE:
            blobs = [_dense_text(rng, rng.randint(1, 5)).encode("utf-8") for _ in range(600)]
        else:
            blobs = [(rng.choice(LONG_WORDS).encode() if i % 9 == 4 else b"") for i in range(600)]
            blobs[100] = "́́".encode("utf-8")
        blobs[1] = b"ab " + CUT
        blobs[2] = b""
        for i in range(3, 600):                        # shorten until the filler string has room
            if sum(map(len, blobs)) - len(blobs[599]) <= 2960:
                break
            blobs[i] = blobs[i][:1] if content == DENSE else b""
        return Batch(size, content, _fit(blobs, 599, content, 3001))
    if size == "M":                                    # 9 strings, tile + 37 bytes: the filler string crosses the tile edge
        blobs = _strings(rng, content, 3, 200, 500)
        blobs = [blobs[0], b"ab " + CUT, blobs[1]] + (_extras(content)[:3] if content == SPARSE else [blobs[2][:40], b"", b"q"]) + [b"", b"", b""]
        blobs[6] = b"x y" if content == DENSE else LONG_WORDS[40].encode()
        blobs[8] = b"z" if content == DENSE else "́́́".encode("utf-8")
        assert len(blobs) == 9
        return Batch(size, content, _with_edges(_fit(blobs, 7, content, tile + 37), 7, content, tile))
    if size == "M5":                                   # about 70 strings, 5 tiles + 11 bytes
        blobs = _strings(rng, content, 64 if content == SPARSE else 70, 100, 420)
        blobs[1:1] = [b"ab " + CUT]
        blobs[20:20] = _extras(content)
        keep, used = [], 0
        for b in blobs:                                # leave two tiles to the filler string: it then crosses at least one edge
            if used + len(b) > 3 * tile:
                b = b[:7].decode("utf-8", "ignore").encode("utf-8")
            keep.append(b)
            used += len(b)
        keep.append(b"")
        return Batch(size, content, _with_edges(_fit(keep, len(keep) - 1, content, 5 * tile + 11), len(keep) - 1, content, tile))
    if size == "L":                                    # just over the small route's character limit: small_chars + 37 chars
        want_chars = small_chars + 37
        pool = _strings(rng, content, 400, 0, 180)
        pool[7:7] = _extras(content)
        blobs, chars, k = [b"xy", b"ab " + CUT], 6, 0
        while True:
            nxt = pool[k % len(pool)]
            n_chars = len(nxt.decode("utf-8"))
            if chars + n_chars > want_chars - 64:
                break
            blobs.append(nxt)
            chars += n_chars
            k += 1
        blobs.append(_filler(content, want_chars - chars))
        b = Batch(size, content, blobs)
        if b.total_bytes % 64 == 0:                    # the end must not sit on a word edge: one ASCII letter becomes a 2-byte letter
            blobs[-1] = blobs[-1][:-1] + "\xe9".encode("utf-8")
            b = Batch(size, content, blobs)
        return b
    raise ValueError(size)


def build_batches(tile, small_chars, small_strings, sizes=SIZE_NAMES):
    """{(size, content): Batch} for both contents of every size"""
    return {(s, c): build_batch(s, c, tile, small_chars, small_strings) for s in sizes for c in (DENSE, SPARSE)}


# ---- the reference of one batch ------------------------------------------------------------------------------------------------------
def _csr(rows):
    """rows of (key, value) pairs -> the canonical CSR: distinct keys ascending as signed int32, values summed (a sum of 0 is kept)"""
    indptr, indices, data = [0], [], []
    for row in rows:
        c = collections.Counter()
        for key, v in row:
            c[key] += v
        for key in sorted(c):
            indices.append(key)
            data.append(c[key])
        indptr.append(len(indices))
    return np.array(indptr, np.int64), np.array(indices, np.int32), np.array(data, np.int32)


class Reference:
    """Every result of one batch, from the oracle's split values and parse matrix of its code points.  ``tables`` = (C_SPLIT, C_MASK,
    C_SYM) for run-time rules, None for the built-in ones.  ``form`` picks the code points: "cps" (the decoded text, which is also what
    byte space reports mapped to byte positions), "k1", "k2"."""

    def __init__(self, oracle, batch, tables=None, form="cps"):
        self.b = b = batch
        cps = np.ascontiguousarray({"cps": b.cps, "k1": b.k1, "k2": b.k2}[form], np.uint32)
        n = cps.size
        row = b.row
        m = oracle.gen_parse_matrix_batch(cps, row) if n else np.zeros((0, 25), np.int8)
        self.matrix = m
        if tables is None:
            vals, bits = oracle.split_batch(cps, row)
            self.values = vals
        else:
            self.values = oracle.split_values_rules_batch(cps, row, *tables, m=m).view(np.uint8) if n else np.zeros(0, np.uint8)
        bound = self.values != 0
        self.cp_mask = self._bits(bound, n)
        space = m[:, 5] != 0
        g = np.flatnonzero(bound)                                  # every boundary, as a packed char index
        s_of = np.searchsorted(row, g, side="right") - 1            # its string
        ends = np.minimum(np.append(g[1:], n), row[s_of + 1]) if g.size else g
        self.off_counts = np.bincount(s_of, minlength=b.n_str).astype(np.int64)[:b.n_str] if b.n_str else np.zeros(0, np.int64)
        self.offsets = g - row[s_of]
        ns = np.flatnonzero(~space)                                 # chars that str.strip() keeps
        lo, hi = np.searchsorted(ns, g, side="left"), np.searchsorted(ns, ends, side="left")
        kept = hi > lo
        self.tok_str = s_of[kept]
        raw0, raw1 = g[kept], ends[kept]
        st0 = ns[lo[kept]] if kept.any() else raw0
        st1 = ns[hi[kept] - 1] + 1 if kept.any() else raw1
        base = row[self.tok_str]
        self.counts = np.bincount(self.tok_str, minlength=b.n_str).astype(np.int64)[:b.n_str] if b.n_str else np.zeros(0, np.int64)
        self.spans = np.stack([st0 - base, st1 - base], axis=1).reshape(-1, 2)
        self.spans4 = np.stack([raw0 - base, raw1 - base, st0 - base, st1 - base], axis=1).reshape(-1, 4)
        csum = np.zeros((n + 1, 25), np.uint64)
        if n:
            np.cumsum(m.view(np.uint8), axis=0, dtype=np.uint64, out=csum[1:])
        self.feats = (csum[raw1] - csum[raw0]).astype(np.uint8).view(np.int8).reshape(-1, 25)
        self.n_tokens = int(kept.sum())
        if form != "cps":
            return
        # byte space: a char's position is its lead byte, an end position the next char's lead byte (the byte total behind the last)
        pos = np.append(b.lead, b.total_bytes).astype(np.int64)
        bbase = b.boff[self.tok_str]
        byte_bound = np.zeros(b.total_bytes, bool)
        byte_bound[pos[g]] = True
        self.byte_mask = self._bits(byte_bound, b.total_bytes)
        self.byte_offsets = pos[g] - b.boff[s_of]
        self.byte_spans = np.stack([pos[st0] - bbase, pos[st1] - bbase], axis=1).reshape(-1, 2)
        self.byte_spans4 = np.stack([pos[raw0] - bbase, pos[raw1] - bbase, pos[st0] - bbase, pos[st1] - bbase], axis=1).reshape(-1, 4)
        self._tokens = None

    @staticmethod
    def _bits(flags, total):
        return np.packbits(np.concatenate([flags, np.zeros((-total) % 64, bool)]), bitorder="little").view(np.uint64)

    @property
    def tokens(self):
        """the byte slice of every token, in rank order"""
        if self._tokens is None:
            raw = self.b.u8.tobytes()
            a = (self.byte_spans[:, 0] + self.b.boff[self.tok_str]).tolist()
            e = (self.byte_spans[:, 1] + self.b.boff[self.tok_str]).tolist()
            self._tokens = [raw[x:y] for x, y in zip(a, e)]
        return self._tokens

    def rows(self):
        """the tokens string by string"""
        out, k = [], 0
        for c in self.counts.tolist():
            out.append(self.tokens[k:k + c])
            k += c
        return out

    def grams(self, min_n, max_n, sep):
        """the grams of every string, order by order"""
        sep = bytes([sep])
        return [[sep.join(t[i:i + n]) for n in range(min_n, max_n + 1) for i in range(len(t) - n + 1)] for t in self.rows()]

    def join(self, sep):
        rows = [bytes([sep]).join(t) for t in self.rows()]
        off = np.zeros(len(rows) + 1, np.int64)
        np.cumsum([len(r) for r in rows], out=off[1:])
        return np.frombuffer(b"".join(rows), np.uint8), off

    def vocab_csr(self, vocab, min_n=1, max_n=1, sep=32):
        """(indptr, indices, data, oov, n_grams) of the vocabulary form against the dict ``vocab``"""
        rows, oov, total = [], [], 0
        for gr in self.grams(min_n, max_n, sep):
            rows.append([(vocab[x], 1) for x in gr if x in vocab])
            oov.append(len(gr) - len(rows[-1]))
            total += len(gr)
        return _csr(rows) + (np.array(oov, np.int64), total)

    def hashed_csr(self, hash32, n_features, alternate_sign, min_n=1, max_n=1, sep=32):
        """(indptr, indices, data, n_grams) of the hashed form: h as int32, column |h| mod n_features, sign of h if alternate_sign"""
        rows, total, memo = [], 0, {}
        for gr in self.grams(min_n, max_n, sep):
            row = []
            for x in gr:
                if x not in memo:
                    h = hash32(x)
                    h = h - (1 << 32) if h >= (1 << 31) else h
                    memo[x] = (abs(h) % n_features, -1 if h < 0 else 1)
                col, sign = memo[x]
                row.append((col, sign if alternate_sign else 1))
            rows.append(row)
            total += len(gr)
        return _csr(rows) + (total,)


def reference(oracle, batch, tables=None, form="cps", name=None):
    """the cached Reference of a batch (``name`` names the tables in the cache key)"""
    key = (name if tables is not None else None, form)
    if key not in batch._ref:
        batch._ref[key] = Reference(oracle, batch, tables, form)
    return batch._ref[key]
