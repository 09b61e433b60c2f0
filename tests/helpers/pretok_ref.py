"""GPT-2's pre-tokenizer in byte space, restated in plain Python over ``bytes`` from the definition in include/latok_hip.h
(latok_pretokens_utf8_bytes_batch).  It shares no code with latok_amd/csrc/pretok.h, and it reads its character classes from
tests/golden/pretok_classes.json, never from the ``unicodedata`` of the interpreter that runs it.

    starts(b)      the byte offsets at which a pre-token starts (ascending; empty for b"")
    pretokens(b)   the byte ranges [(a, e), ...]: every byte of b lies in exactly one
"""
import bisect
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "pretok_classes.json")
CONTRACTIONS = (b"s", b"t", b"re", b"ve", b"m", b"ll", b"d")
_tables = None


def tables():
    global _tables
    if _tables is None:
        with open(GOLDEN) as f:
            g = json.load(f)
        _tables = {"version": g["unicode_version"]}
        for k in "LNS":
            _tables[k] = ([r[0] for r in g[k]], [r[1] for r in g[k]])
    return _tables


def _in(k, cp):
    lo, hi = tables()[k]
    i = bisect.bisect_right(lo, cp) - 1
    return i >= 0 and cp <= hi[i]


def cp_class(cp):
    """'S', 'L', 'N' or 'O' of a scalar value"""
    return "S" if _in("S", cp) else "L" if _in("L", cp) else "N" if _in("N", cp) else "O"


def char_starts(b):
    return [i for i in range(len(b)) if i == 0 or (b[i] & 0xC0) != 0x80]


def char_class(c):
    """the class of one character's bytes: that of its code point if they are exactly one well-formed sequence, else 'O'"""
    try:
        s = bytes(c).decode("utf-8")   # (strict: no overlong form, no surrogate, nothing above U+10FFFF)
    except UnicodeDecodeError:
        return "O"
    return cp_class(ord(s)) if len(s) == 1 else "O"


def starts(b):
    n = len(b)
    if n == 0:
        return []
    cs = char_starts(b)
    ends = cs[1:] + [n]
    cls = [char_class(b[s:e]) for s, e in zip(cs, ends)]
    is_start = set(cs)
    inside, forced = set(), set()
    for i, s in enumerate(cs):                       # rule 1
        if b[s] != 0x27 or ends[i] != s + 1:
            continue
        prev_space = i > 0 and cls[i - 1] == "S" and b[cs[i - 1]:ends[i - 1]] == b" "
        if not (i == 0 or cls[i - 1] in "LN" or (cls[i - 1] == "S" and not prev_space)):
            continue
        for w in CONTRACTIONS:
            k = 1 + len(w)
            if b[s + 1:s + k] == w and (s + k == n or s + k in is_start):   # the letters are whole characters of this string
                inside.update(range(s + 1, s + k))
                if s + k < n:
                    forced.add(s + k)
    out = []
    for i, s in enumerate(cs):
        if s in inside:
            continue
        first, force = i == 0, s in forced
        if cls[i] == "S":                            # rule 2
            if first or force or cls[i - 1] != "S" or (i + 1 < len(cs) and cls[i + 1] != "S"):
                out.append(s)
        else:                                        # rule 3
            if first or force:
                out.append(s)
            elif cls[i - 1] == "S":
                if b[cs[i - 1]:ends[i - 1]] != b" ":
                    out.append(s)
            elif cls[i - 1] != cls[i]:
                out.append(s)
    return out


def pretokens(b):
    st = starts(b)
    return list(zip(st, st[1:] + [len(b)]))


ALPHABET = ["'", "'", " ", " ", " ", "\n", "\t", "s", "t", "r", "e", "v", "m", "l", "d", "a", "Z", "0", "7", "é", "　", "日", "本",
            "!", ".", " ", "²", "\U0001F913", "\U0001D7D8", "\r", " ", "x", "-"]


def random_text(rng, max_chars=24):
    return "".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, max_chars)))
