"""Content, reference and census for the featurize kernel (k_features_tiles / feature_tile, latok_amd/csrc/feature_kernels.hip).

Three parts, none of which calls the product's kernels:
  * ``batch_reference`` / ``reference``: what featurize must return for a batch -- counts, spans4 and the 25 sums -- from the
    oracle alone: its parse matrix string by string, summed (uint8 wrap) over the tokens cut at its boundaries, ``str.strip`` and
    drop-empty.  It is ``span_strip_content.reference`` over arrays (a sweep of 0x110000 code points holds values that no ``str``
    can, and millions of tokens); tests/test_featurize_content.py holds it equal to that function.
  * ``census``: the set of classes (names below) a batch reaches inside feature_tile, from the reference alone: kept token starts
    in the packed code-point layout, 4096-char tiles, 64-char words.  The kernel's constants come from the built library
    (``limits``: latok_debug_limits, no device needed), the span rounds are derived from kFeatWinBytes as span_round<OUT>() does.
  * ``batches``: deterministic builders that plant every class of ``REQUIRED``.

Two things the arithmetic of the form choice rules out, so that no class asks for them:
  * a word-major tile of three or more rounds: word-major needs maxc * 2 * rounds <= ceil(n / 64) * kFeatFormThresh, and the fullest
    word holds at least n / 64 tokens, so rounds <= kFeatFormThresh / 2 = 2.5;
  * for the same reason a two-round word-major tile sits within 0.8 of the threshold; "at least 2x away" is asked of WM_1, TM_1 and
    TM_MULTI only.
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import span_strip_content as ssc  # noqa: E402

TILE = ssc.TILE
ALPHA, SPACE, SYMBOL, PREV_ALPHA, PREV_SPACE, PREV_SYMBOL = 0, 5, 6, 12, 18, 20      # latok_amd/core/offsets.py
_NONE = np.zeros((0, 1), np.int8)
# every char that is a space, a letter or a symbol, or stands behind one, opens a token: with the interleavings of
# test_gpu_unicode_sweep._variants each char is a token of its own
SWEEP_TABLE = (np.array([[SPACE], [PREV_SPACE], [ALPHA], [PREV_ALPHA], [SYMBOL], [PREV_SYMBOL]], np.int8), _NONE, _NONE)
N_CP = 0x110000
_WS_TAB = None


def ws_table():
    """bool[N_CP + 1]: str.isspace() of every code point; the last entry stands for values no str can hold"""
    global _WS_TAB
    if _WS_TAB is None:
        t = np.zeros(N_CP + 1, bool)
        t[[c for c in range(N_CP) if chr(c).isspace()]] = True
        _WS_TAB = t
    return _WS_TAB


def limits():
    """the constants of k_features_tiles from the built library, and the span rounds as span_round<OUT>() derives them"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(14, np.int64)
    assert fn(out.ctypes.data, 14) == 14
    v = out.tolist()
    lim = {"TILE": v[0], "SMALL_CHARS": v[6], "SMALL_STRINGS": v[7], "WAVES": v[9], "R": v[10], "RTM": v[11], "THRESH": v[12], "WIN": v[13]}
    lim["SR64"], lim["SR32"] = min(lim["WIN"] // 32, lim["R"]), min(lim["WIN"] // 16, lim["R"])
    assert lim["TILE"] == TILE
    return lim


# ---- reference -----------------------------------------------------------------------------------------------------------
def batch_reference(oracle, cps, row, tables, unit):
    """ssc.reference for a packed batch (uint32 code points, int64 row offsets in chars); unit: positions in chars or UTF-8 bytes.
    Besides the fields of ssc.Reference (without .tokens) it keeps the code-point layout for the census."""
    assert unit in ssc.UNITS
    cps = np.ascontiguousarray(cps, np.uint32)
    row = np.ascontiguousarray(row, np.int64)
    r = ssc.Reference()
    n, total = row.size - 1, int(row[-1])
    r.unit, r.n_str, r.total_chars, r.row_cp = unit, n, total, row
    m = oracle.gen_parse_matrix_batch(cps, row)
    if tables is None:
        vals = oracle.split_batch(cps, row, want_bits=False)[0]
    else:
        vals = oracle.split_values_rules_batch(cps, row, *tables, m=m)
    nz = np.nonzero(vals)[0]
    ends = np.append(nz[1:], total)
    sid = np.searchsorted(row, nz, "right") - 1
    assert nz.size == 0 or (ends <= row[sid + 1]).all()          # every string opens with a boundary: no token crosses strings
    nonws = ~ws_table()[np.minimum(cps, N_CP)]
    idx = np.arange(total, dtype=np.int64)
    nxt = np.minimum.accumulate(np.where(nonws, idx, total)[::-1])[::-1] if total else idx       # first non-space char at or behind i
    prv = np.maximum.accumulate(np.where(nonws, idx + 1, 0)) if total else idx                   # end of the last one at or before i
    c = nxt[nz]
    kept = c < ends
    d = prv[ends - 1]
    if unit == "bytes":
        w = cps.astype(np.int64)
        pos = np.zeros(total + 1, np.int64)
        np.cumsum(1 + (w >= 0x80) + (w >= 0x800) + (w >= 0x10000), out=pos[1:])
    else:
        pos = np.arange(total + 1, dtype=np.int64)
    r.row = pos[row]
    r.total = int(pos[-1])
    base = r.row[sid]
    r.spans4 = np.stack([pos[nz] - base, pos[ends] - base, pos[c] - base, pos[d] - base], axis=1)[kept].reshape(-1, 4)
    r.spans = np.ascontiguousarray(r.spans4[:, 2:])
    sums = np.add.reduceat(m.view(np.uint8), nz, axis=0, dtype=np.uint8).view(np.int8) if nz.size else np.zeros((0, 25), np.int8)
    r.feats = np.ascontiguousarray(sums[kept]).reshape(-1, 25)
    r.counts = np.bincount(sid[kept], minlength=n).astype(np.int64)
    r.bound_counts = np.bincount(sid, minlength=n).astype(np.int64)
    r.offsets = pos[nz] - base
    r.empty = (row[1:] == row[:-1]).tolist()
    # the code-point layout
    r.bnd, r.kp, r.ke, r.nonws, r.alpha, r.wide = nz, nz[kept], ends[kept], nonws, m[:, ALPHA] != 0, cps >= 0x80
    return r


def pack(texts):
    cps = np.frombuffer("".join(texts).encode("utf-32-le", "surrogatepass"), "<u4").astype(np.uint32)
    row = np.zeros(len(texts) + 1, np.int64)
    np.cumsum([len(t) for t in texts], out=row[1:])
    return cps, row


def reference(oracle, texts, tables, unit):
    return batch_reference(oracle, *pack(texts), tables, unit)


def first_diff(got, r, lim):
    """the first token whose record or sums differ, with its tile, word and the classes of its tile: for the failure message"""
    counts, spans4, feats = got
    if not np.array_equal(counts, r.counts):
        s = int(np.nonzero(counts != r.counts)[0][0]) if counts.shape == r.counts.shape else -1
        return "counts differ first at string %d" % s
    k = min(len(spans4), len(r.spans4))
    bad = (spans4.reshape(-1, 4)[:k] != r.spans4[:k]).any(axis=1) | (feats.reshape(-1, 25)[:k] != r.feats[:k]).any(axis=1)
    if not bad.any():
        return "lengths differ: %d / %d" % (len(spans4), len(r.spans4))
    j = int(np.nonzero(bad)[0][0])
    p, e = int(r.kp[j]), int(r.ke[j])
    cols = np.nonzero(feats[j] != r.feats[j])[0].tolist()
    t = p // TILE
    sel = (r.kp // TILE) == t
    cnt = np.bincount(r.kp[sel] // 64 - t * 64, minlength=64)
    sub = _tile_classes(r, lim, t, cnt, int(np.searchsorted(r.kp, t * TILE)))
    own = _token_classes(r, j, _form(int(cnt.sum()), int(cnt.max()), lim)[0], cnt, set(r.row_cp.tolist())) if e >= p // 64 * 64 + 64 else set()
    return ("token %d: tile %d word %d bit %d, raw [%d, %d) of %d chars; spans4 %s want %s; sums differ in columns %s: %s want %s; token classes %s; tile classes %s"
            % (j, t, p % TILE // 64, p % 64, p, e, r.total_chars, spans4[j].tolist(), r.spans4[j].tolist(), cols,
               feats[j][cols].tolist(), r.feats[j][cols].tolist(), sorted(own), sorted(sub)))


# ---- census --------------------------------------------------------------------------------------------------------------
def _form(n, maxc, lim):
    """(token-major?, form quantity, threshold) of a tile of n tokens whose fullest word holds maxc: feature_tile's choice"""
    q = maxc * 2 * ((n + lim["R"] - 1) // lim["R"])
    thr = (n + 63) // 64 * lim["THRESH"]
    return q > thr, q, thr


def _tile_classes(r, lim, t, cnt, base_out):
    """families 1-5 and 12: the classes of tile t; cnt = kept token starts per word, base_out = rank of its first token"""
    got = set()
    R, RTM = lim["R"], lim["RTM"]
    n, maxc = int(cnt.sum()), int(cnt.max())
    if n == 0:
        return got
    tm, q, thr = _form(n, maxc, lim)
    off = np.concatenate([[0], np.cumsum(cnt)])
    wide = bool(r.wide[t * TILE:(t + 1) * TILE].any())
    form = None
    if not tm:
        if n <= R and 2 * q <= thr:
            form = "WM_1"
        if n > R:
            form = "WM_MULTI"
        if _form(n + 1, maxc + 1, lim)[0]:
            got.add("NEAR_BELOW")
        if lim["SR64"] < n <= R:
            got.add("SPAN64:INSIDE_ONE_FEATURE_ROUND")
        if n > 2 * lim["SR64"] + 1:
            got.add("SPAN64:THREE_ROUNDS")
        for name, sr in (("SPAN64", lim["SR64"]), ("SPAN32", lim["SR32"])):
            for edge in range(sr, n, sr):
                w = int(np.searchsorted(off, edge, "right")) - 1
                if off[w] < edge:
                    got.add(name + ":WORD_SPLIT")
        for edge in range(R, n, R):        # the round ends in front of the token of rank `edge`
            w = int(np.searchsorted(off, edge, "right")) - 1
            j = edge - int(off[w])
            if j == 0:
                got.add("WM_EDGE:BETWEEN_WORDS")
                continue
            wb = t * TILE + 64 * w
            bits = r.kp[base_out + int(off[w]):base_out + int(off[w + 1])] - wb
            bnd = r.bnd[np.searchsorted(r.bnd, wb):np.searchsorted(r.bnd, wb + 32)] - wb      # all boundaries of the low half
            low = int((bits < 32).sum())
            strad = low - 1 if low and bnd.max() == bits[low - 1] else -1                      # the last low token, nothing cut behind it
            if strad == j - 1:
                got.add("WM_EDGE:STRADDLER_LAST_SLOT")
            elif strad == j:
                got.add("WM_EDGE:STRADDLER_FIRST_SLOT")
            elif bits[j] < 32:
                got.add("WM_EDGE:LOW_HALF")
            elif bits[j - 1] >= 32:
                got.add("WM_EDGE:HIGH_HALF")
    else:
        if 2 * thr <= q:
            form = "TM_1" if n <= RTM else "TM_MULTI"
        if n == TILE:
            got.add("TM_FULL_TILE")
        if not _form(n - 1, maxc - 1, lim)[0]:
            got.add("NEAR_ABOVE")
        for edge in range(RTM, n, RTM):
            w = int(np.searchsorted(off, edge, "right")) - 1
            got.add("TM_EDGE:WORD_SPLIT" if off[w] < edge else "TM_EDGE:WORD_AT_EDGE")
    if form:
        got.add(form)
        if wide:
            got.add("MB:" + form)
    rnd = RTM if tm else R
    for win0 in range(0, n, rnd):
        shift = (base_out + win0) * 25 % 16
        nb = min(rnd, n - win0) * 25
        head = min((16 - shift) & 15, nb)
        got.add("SHIFT:%d" % shift)
        if (nb - head) >> 4 == 0:
            got.add("SHIFT:HEAD_AND_TAIL_ONLY")
        if nb % 16 == 1:
            got.add("SHIFT:BYTES_16K_PLUS_1")
    if n == 1:
        got.add("SHIFT:SINGLE_TOKEN_TILE")
    return got


def _token_classes(r, j, tm, cnt, row_set):
    """families 6, 7, 8, 11 and 13: the classes of kept token j, which leaves its word; tm, cnt: the form and the tokens per word of
    its tile"""
    got, total = set(), r.total_chars
    p, e = int(r.kp[j]), int(r.ke[j])
    b = p // 64 * 64
    t = p // TILE
    t0, d = t * TILE, e - p
    frm = t0 + TILE + 64                           # where the whole-wave walk begins
    half = "LOW" if p % 64 < 32 else "HIGH"
    end = []
    if e < total:
        we, tile_end_word = e // 64, (t + 1) * 64
        if we < tile_end_word:
            k = we - p // 64
            end += ["WORD+%d" % k] if k in (1, 2, 62, 63) else []
        elif we == tile_end_word:
            end += ["NEXT_TILE_WORD0_BIT%d" % (e % 64)] if e % 64 in (0, 63) else []
        else:
            if we == tile_end_word + 1:
                end.append("NEXT_TILE_WORD1")
            step = (e - frm) // TILE
            end.append("WALK_STEP%s" % ("1" if step == 0 else "2" if step == 1 else "3+"))
            if e > frm and (e - frm) % TILE == 0:
                end.append("WALK_STEP_EDGE")
    if d > 64:
        got |= {"LEAVE:%s:%s" % (half, x) for x in end}
    if tm:
        if e < b + 128 and e > b + 64 and cnt[(b - t0) // 64] >= 2:
            got.add("TM_SPAN:NEXT_WORD_SHARED_CARRY")
        if e >= b + 128:
            got.add("TM_SPAN:FAR")
    if (e - 1) // TILE > t and int(r.nonws[p:e].sum()) >= 256:
        got.add("WRAP:CROSSES_TILE")
    if e in row_set and e < total and r.alpha[e] and r.nonws[e - 1]:      # family 7: the string ends here, a letter behind the edge
        rel = e - t0
        if rel in (TILE, TILE + 1, TILE + 64, TILE + 65):
            got.add("STR_END:TILE+%d" % rel)
        if e > frm + 1:
            if e % 64 in (0, 1, 2, 63):
                got.add("STR_END:WALK_WORD_OFFSET_%d" % (e % 64))
            if e - frm >= TILE and (e - frm) % TILE in (0, 1):
                got.add("STR_END:WALK_STEP_EDGE+%d" % ((e - frm) % TILE))
    if e == total:                                                        # family 8
        got.add("LAST:NEXT_WORD" if e <= b + 128 and e <= t0 + TILE else "LAST:NEXT_TILE_WORD0" if e < t0 + TILE + 64 else
                "LAST:WALK" if e > frm else "LAST:OTHER")
    return got


def census(oracle, texts, tables, lim, ref=None):
    """the classes a batch reaches"""
    r = ref if ref is not None else reference(oracle, texts, tables, "chars")
    got = set()
    total = r.total_chars
    if total == 0:
        return got
    n_tiles = (total + TILE - 1) // TILE
    cnt = np.bincount(r.kp // 64, minlength=n_tiles * 64).reshape(n_tiles, 64)
    n_t = cnt.sum(axis=1)
    base_out = np.concatenate([[0], np.cumsum(n_t)])
    tm_tile = np.zeros(n_tiles, bool)
    for t in range(n_tiles):
        if n_t[t]:
            tm_tile[t] = _form(int(n_t[t]), int(cnt[t].max()), lim)[0]
            got |= _tile_classes(r, lim, t, cnt[t], int(base_out[t]))
        elif n_t[:t].any() and n_t[t + 1:].any() and (t + 1) * TILE <= total:      # family 10
            inside = r.nonws[t * TILE:(t + 1) * TILE]
            if inside.all():
                got.add("EMPTY_TILE:INSIDE_A_TOKEN")
            if not inside.any():
                got.add("EMPTY_TILE:WHITESPACE")
    # families 6, 7, 8, 11, 13: the tokens that leave their word
    row_set = set(r.row_cp.tolist())
    for j in np.nonzero(r.ke >= r.kp // 64 * 64 + 64)[0].tolist():
        t = int(r.kp[j]) // TILE
        got |= _token_classes(r, j, bool(tm_tile[t]), cnt[t], row_set)
    if r.kp.size and r.ke[-1] == total and r.ke[-1] <= r.kp[-1] // 64 * 64 + 64 and r.ke[-1] % 64:
        got.add("LAST:OWN_WORD")
    if total % TILE in (1, 63, 64, 65, 4095, 0):
        got.add("TAIL:%d" % (total % TILE))
    # family 9: string starts
    vals, reps = np.unique(r.row_cp, return_counts=True)
    for v in vals[reps >= 66].tolist():                # >= 65 empty strings at one offset
        if v < total and n_t[v // TILE] and v % TILE in (0, TILE - 1):
            got.add("EMPTY_RUN:TILE_%s_CHAR" % ("FIRST" if v % TILE == 0 else "LAST"))
        if v % TILE == 127 and v > TILE and n_t[v // TILE - 1]:
            got.add("EMPTY_RUN:TILE+4223")
    starts = np.zeros(n_tiles * TILE, bool)
    starts[vals[vals < total]] = True
    if starts.reshape(n_tiles, TILE).all(axis=1).any():
        got.add("STARTS:ONE_CHAR_STRINGS_FILL_A_TILE")
    if (starts[r.kp] & (r.kp % 64 == 63)).any():
        got.add("STARTS:BIT63_WITH_TOKEN")
    return got


_ENDS = ["WORD+1", "WORD+2", "WORD+62", "WORD+63", "NEXT_TILE_WORD0_BIT0", "NEXT_TILE_WORD0_BIT63", "NEXT_TILE_WORD1", "WALK_STEP1",
         "WALK_STEP2", "WALK_STEP3+", "WALK_STEP_EDGE"]
FAMILIES = {
    1: ["WM_1", "WM_MULTI", "TM_1", "TM_MULTI", "TM_FULL_TILE", "NEAR_BELOW", "NEAR_ABOVE"],
    2: ["SPAN64:INSIDE_ONE_FEATURE_ROUND", "SPAN64:THREE_ROUNDS", "SPAN64:WORD_SPLIT", "SPAN32:WORD_SPLIT"],
    3: ["WM_EDGE:LOW_HALF", "WM_EDGE:STRADDLER_LAST_SLOT", "WM_EDGE:STRADDLER_FIRST_SLOT", "WM_EDGE:HIGH_HALF"],
    4: ["TM_EDGE:WORD_SPLIT", "TM_EDGE:WORD_AT_EDGE"],
    5: ["SHIFT:%d" % s for s in range(16)] + ["SHIFT:SINGLE_TOKEN_TILE", "SHIFT:HEAD_AND_TAIL_ONLY", "SHIFT:BYTES_16K_PLUS_1"],
    6: ["LEAVE:%s:%s" % (h, x) for h in ("LOW", "HIGH") for x in _ENDS],
    7: ["STR_END:TILE+%d" % x for x in (4096, 4097, 4160, 4161)] + ["STR_END:WALK_WORD_OFFSET_%d" % x for x in (0, 1, 2, 63)] +
       ["STR_END:WALK_STEP_EDGE+0", "STR_END:WALK_STEP_EDGE+1"],
    8: ["TAIL:%d" % x for x in (1, 63, 64, 65, 4095, 0)] + ["LAST:OWN_WORD", "LAST:NEXT_WORD", "LAST:NEXT_TILE_WORD0", "LAST:WALK"],
    9: ["EMPTY_RUN:TILE_FIRST_CHAR", "EMPTY_RUN:TILE_LAST_CHAR", "EMPTY_RUN:TILE+4223", "STARTS:ONE_CHAR_STRINGS_FILL_A_TILE",
        "STARTS:BIT63_WITH_TOKEN"],
    10: ["EMPTY_TILE:INSIDE_A_TOKEN", "EMPTY_TILE:WHITESPACE"],
    11: ["WRAP:CROSSES_TILE"],
    12: ["MB:WM_1", "MB:WM_MULTI", "MB:TM_1", "MB:TM_MULTI"],
    13: ["TM_SPAN:NEXT_WORD_SHARED_CARRY", "TM_SPAN:FAR"],
}
REQUIRED = frozenset(c for f in FAMILIES.values() for c in f)
# what fits a batch of at most kSmallChars bytes (`mid` and the tails): the families that need no long token
REQUIRED_SMALL = frozenset(c for k in (1, 2, 3, 4, 8, 12, 13) for c in FAMILIES[k])


# ---- content -------------------------------------------------------------------------------------------------------------
_FILL = "lorem ipsum, dolor sit amet. Consectetur #adipiscing elit; sed do 12 eiusmod "


class _Builder:
    """strings of a batch, with the global code-point position of what comes next"""

    def __init__(self):
        self.strings, self.cur, self.pos = [], [], 0

    def add(self, s):
        self.cur.append(s)
        self.pos += len(s)

    def end(self):
        self.strings.append("".join(self.cur))
        self.cur = []

    def empties(self, k):
        self.end()
        self.strings += [""] * k

    def fill(self, n):
        """n chars of ordinary text that end with a symbol: what follows opens a token at its own first char (behind a space the
        token would begin at the space)"""
        if n:
            self.add((_FILL * (n // len(_FILL) + 1))[:n - 1] + ",")

    def to(self, at, mod=TILE):
        self.fill((at - self.pos) % mod)
        assert self.pos % mod == at % mod

    def tile(self, text):
        """text from a tile's first char on, a whole number of tiles"""
        assert len(text) % TILE == 0
        self.to(0)
        self.add(text)


def _word(k, ch="a"):
    """64 chars that hold k tokens, each a space and letters, starting at bits 0, n, 2n, ... (the last takes the remainder)"""
    n = 64 // k
    return (" " + ch * (n - 1)) * (k - 1) + " " + ch * (64 - n * (k - 1) - 1)


def _p15(ch="a"):
    """64 chars, 15 tokens: 8 start in the low half, the last of them (bit 28) reaches bit 35, 7 start in the high half"""
    return (" " + ch * 3) * 7 + " " + ch * 7 + (" " + ch * 3) * 7


def _forms(b, a=("a", ",", ".")):
    """family 1 (and 2): one tile of each form, with the letter and the two symbol chars given"""
    L, s1, s2 = a
    b.tile((" " + L * 3) * 1024)                                   # 1024 tokens, 16 per word: word-major, two rounds
    b.tile(((" " + L * 4) * 820)[:TILE])                           # 819 tokens: one feature round, two int64 span rounds
    b.tile(((" " + L * 2) * 20 + (" " + L) * 2) * 64)              # 1408 tokens, 22 per word: three int64 span rounds
    b.tile((s1 + s2) * 2048)                                       # 4096 tokens: token-major, the full tile
    b.tile((s1 + s2) * 32 + _word(8, L) * 63)                      # one dense word among sparse ones: token-major, one round
    b.tile(_word(8, L) * 64)                                       # 512 tokens, 8 per word: word-major, far below the threshold
    b.tile(_word(7, L) + _word(2, L) * 63)                         # one token below the threshold
    b.tile(_word(8, L) + _word(2, L) * 63)                         # ... and one above
    b.fill(64)


def _round_edges(b, lim):
    """families 3 and 4"""
    for j in (3, 7, 8, 12):                                        # slot inside its word of the first token of the second round
        s = (j - lim["R"]) % 15                                    # tokens taken out of the tile's first word
        b.tile(_word(15 - s) + _p15() * 63)
    b.tile(_word(8) + ",." * 2016)                                 # the token-major round ends inside a word
    b.fill(64)


def _shifts(b):
    """family 5: 17 tokens per tile move the rank of the next tile's first token by 1 mod 16"""
    for _ in range(17):
        b.tile((" " + "a" * 239) * 16 + " " + "a" * 255)
    for _ in range(5):                                             # single tokens at ranks r .. r + 4: one of them has no 16-byte vector
        b.tile(" " + "a" * 4095)
    b.tile((" " + "a" * 454) * 8 + " " + "a" * 455)                # 9 tokens: 225 bytes
    b.fill(64)


def _leavers(b):
    """families 6 and 11: long runs of letters from the low and the high half of a word"""
    for bit in (5, 40):
        for word, end in ((3, 3 * 64 + 75 + bit), (1, 3 * 64 + 10), (1, 63 * 64 + 10), (0, 63 * 64 + 10), (60, TILE), (60, TILE + 63),
                          (60, TILE + 64 + 10), (60, TILE + 64 + 1000), (60, 2 * TILE + 64 + 1000), (60, 3 * TILE + 64 + 1000),
                          (60, 2 * TILE + 64), (10, 4 * TILE + 64)):
            b.to(word * 64 + bit)
            b.add("a" * (end - word * 64 - bit) + " ")


def _string_ends(b):
    """family 7: the string of a carrying token ends at the places the E / E2 bits come from; a letter opens the next string"""
    for end in (TILE, TILE + 1, TILE + 64, TILE + 65, TILE + 64 + 640, TILE + 64 + 641, TILE + 64 + 642, TILE + 64 + 703,
                2 * TILE + 64, 2 * TILE + 65, 3 * TILE + 64, 3 * TILE + 65):
        b.to(62 * 64 + 5)
        b.add("a" * (end - 62 * 64 - 5))
        b.end()
        b.add("bcd ")


def _string_starts(b):
    """family 9"""
    b.to(0)
    b.empties(70)
    b.add("ab cd ")
    b.to(TILE - 1)
    b.empties(70)
    b.add("x yz ")
    b.to(127)
    b.empties(70)
    b.add("ab ")
    b.to(0)
    b.end()
    for i in range(TILE):
        b.add("ab.,1 "[i % 6])
        b.end()
    b.to(63, 64)
    b.end()
    b.add("x yz ")


def _empty_tiles(b):
    """family 10"""
    b.to(100)
    b.add("a" * (3 * TILE) + " ")
    b.fill(200)
    b.add(" " * (3 * TILE))
    b.fill(64)


def _tm_spans(b):
    """family 13: token-major tiles whose tokens end in the next word, and far away"""
    pat = ",." * 10 + "abcde "
    b.tile((pat * (TILE // len(pat) + 1))[:TILE])
    b.tile(",." * 24 + "a" * 200 + " " + ",." * ((TILE - 249) // 2) + " ")
    b.fill(64)


def main_batch(lim, rg="full"):
    """families 1-7 and 9-13 in one batch of more than kSmallChars UTF-8 bytes; the multi-byte tiles stand last, so that all
    positions in front of them are the same in chars and in bytes"""
    b = _Builder()
    b.fill(300)
    _forms(b)
    _round_edges(b, lim)
    _shifts(b)
    _leavers(b)
    _string_ends(b)
    _string_starts(b)
    _empty_tiles(b)
    _tm_spans(b)
    b.end()
    while b.pos < lim["SMALL_CHARS"] + TILE:
        b.fill(997)
        b.end()
    _forms(b, _wide(rg))
    b.end()
    return b.strings


def _wide(rg):
    """(letter, symbol, symbol) of 2, 3 and 4 UTF-8 bytes, as far as the range goes"""
    return ("\xe9", ",", "\xbf") if rg == "latin1" else ("\xe9", "、", "。") if rg == "bmp" else ("日", "、", "\U0001F913")


def mid_batch(lim, rg="full"):
    """families 1-4, 12 and 13 in at most kSmallChars UTF-8 bytes: what the small routes (pinned host batches, the staged UTF-8
    decoder) can be given"""
    b = _Builder()
    b.fill(200)
    _forms(b)
    _round_edges(b, lim)
    _tm_spans(b)
    b.end()
    _forms(b, _wide(rg))
    b.end()
    assert len("".join(b.strings).encode("utf-8")) <= lim["SMALL_CHARS"]
    return b.strings


def tail_batches():
    """family 8: {name: strings}; the batch ends after total mod 4096 = 1, 63, 64, 65, 4095, 0 chars with its last token ending there"""
    out = {}
    for mod, start in ((1, TILE - 30), (63, TILE + 10), (64, TILE + 20), (65, TILE + 10), (4095, TILE + 100), (0, TILE + 4000)):
        b = _Builder()
        b.fill(997)
        b.end()
        b.to(start, 3 * TILE)
        end = {1: TILE + 1, 63: TILE + 63, 64: TILE + 64, 65: TILE + 65, 4095: 4 * TILE - 1, 0: 2 * TILE}[mod]
        b.add("a" * (end - start))
        b.end()
        assert b.pos % TILE == mod
        out["tail%d" % mod] = b.strings
    return out


def padding(lim):
    """ordinary text of a whole number of tiles and more than kSmallChars bytes, to put in front of a small batch"""
    b = _Builder()
    while b.pos < lim["SMALL_CHARS"] + 1:
        b.fill(1000)
        b.end()
    b.to(0)
    b.end()
    return b.strings


def batches(lim, rg="full"):
    """{name: strings}: every batch of the module"""
    out = {"main": main_batch(lim, rg), "mid": mid_batch(lim, rg)}
    out.update(tail_batches())
    return out
