"""The cl100k / Llama 3 pre-tokenizer in byte space, restated in plain Python over ``bytes`` from the definition in include/latok_hip.h
(LATOK_PRETOK_CL100K).  It shares no code with latok_amd/csrc/pretok.h; characters and classes are those of tests/helpers/pretok_ref.py
(tests/golden/pretok_classes.json, never the ``unicodedata`` of the interpreter that runs it).

    starts(b)      the byte offsets at which a pre-token starts (ascending; empty for b"")
    pretokens(b)   the byte ranges [(a, e), ...]: every byte of b lies in exactly one
"""
from helpers.pretok_ref import char_class, char_starts

PATTERN = r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+"
LONG_S = "ſ".encode()
ONE = [bytes([c]) for c in b"stmdSTMD"] + [LONG_S]
TWO = [bytes([a, b]) for x, y in (b"re", b"ve", b"ll") for a in (x, x - 32) for b in (y, y - 32)]
_classes = {}


def _class_of(c):
    """char_class, remembered per character"""
    k = _classes.get(c)
    if k is None:
        k = _classes[c] = char_class(c)
    return k


def starts(b):
    n = len(b)
    if n == 0:
        return []
    cs = char_starts(b)
    ends = cs[1:] + [n]
    chars = [bytes(b[s:e]) for s, e in zip(cs, ends)]
    cls = [_class_of(c) for c in chars]
    m = len(cs)
    nl = [c in (b"\r", b"\n") for c in chars]

    def is_open(i):
        return i == 0 or not (cls[i - 1] == "O" or chars[i - 1] == b" ")

    inside, forced = [False] * m, [False] * m
    for i in range(m):                                   # rule 1
        if chars[i] != b"'" or not is_open(i) or inside[i]:
            continue
        k = 0
        if i + 1 < m and chars[i + 1] in ONE:
            k = 1
        elif i + 2 < m and chars[i + 1] + chars[i + 2] in TWO:
            k = 2
        for j in range(1, k + 1):
            inside[i + j] = True
        if k and i + k + 1 < m:
            forced[i + k + 1] = True
    absorbed, ahead = [False] * m, [False] * m
    for i in range(m):
        absorbed[i] = nl[i] and i > 0 and (cls[i - 1] == "O" or absorbed[i - 1])
    for i in range(m - 1, -1, -1):
        ahead[i] = nl[i] or (cls[i] == "S" and i + 1 < m and cls[i + 1] == "S" and ahead[i + 1])
    out, d = [], 0
    for i in range(m):
        d = d + 1 if i > 0 and cls[i - 1] == "N" else 0  # the N characters directly in front
        if inside[i]:
            continue
        if i == 0 or forced[i]:
            st = True
        elif cls[i] == "L":                              # rule 2
            st = cls[i - 1] == "N" or nl[i - 1] or (cls[i - 1] == "O" and not is_open(i - 1))
        elif cls[i] == "N":                              # rule 3
            st = cls[i - 1] != "N" or d % 3 == 0
        elif cls[i] == "O":                              # rule 4
            st = is_open(i)
        elif absorbed[i]:                                # rule 5
            st = False
        elif cls[i - 1] != "S" or absorbed[i - 1]:
            st = True
        else:
            st = (nl[i - 1] and not ahead[i]) or (i + 1 < m and cls[i + 1] != "S" and not nl[i])
        if st:
            out.append(cs[i])
    return out


def pretokens(b):
    st = starts(b)
    return list(zip(st, st[1:] + [len(b)]))


ALPHABET = ["'", "'", " ", " ", " ", "\n", "\n", "\r", "\t", "s", "t", "r", "e", "v", "m", "l", "d", "S", "T", "R", "E", "V", "M", "L", "D", "ſ", "a",
            "Z", "0", "7", "1", "²", "٣", "३", "\U0001D7D8", "é", "　", "\u0085", "\x1c", "日", "!", ".", "-", "\U0001F913"]


def random_text(rng, max_chars=40):
    return "".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, max_chars)))
