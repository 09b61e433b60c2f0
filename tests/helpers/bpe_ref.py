"""Byte-level BPE, restated from the definition in include/latok_hip.h over ``bytes`` and one ``dict``: the reference the host
harness of bpe.h and the device calls are held to.  It shares no code and no data structure with either: a list of parts, rescanned
whole in every round.  Beside it a tiny byte-pair trainer, which the realistic vocabularies of the tests come from."""
from collections import Counter

# the words of the worked table of the definition, in rank order; the last `b` is a duplicate and is ignored
WORKED_WORDS = [b"a", b"b", b"c", b"d", b"ab", b"cd", b"bc", b"abcd", b"abc", b" ", b" a", b"\xc3", b"\xa9", b"\xc3\xa9", b"adc", b"b"]
# (token, max_bytes, pieces (id, start, end)) with unk = -1
WORKED_CASES = [(b"abcd", 4096, [(7, 0, 4)]), (b"abcb", 4096, [(8, 0, 3), (1, 3, 4)]), (b"bcd", 4096, [(1, 0, 1), (5, 1, 3)]),
                (b" ab", 4096, [(9, 0, 1), (4, 1, 3)]), (b"abab", 4096, [(4, 0, 2), (4, 2, 4)]), (b"adc", 4096, [(14, 0, 3)]),
                (b"adcb", 4096, [(0, 0, 1), (3, 1, 2), (2, 2, 3), (1, 3, 4)]), (b"xab", 4096, [(-1, 0, 1), (4, 1, 3)]),
                (b"abcde", 4096, [(7, 0, 4), (-1, 4, 5)]), (b"a\xc3\xa9", 4096, [(0, 0, 1), (13, 1, 3)]),
                (b"\xa9\xc3", 4096, [(12, 0, 1), (11, 1, 2)]), (b"abc", 2, [(-1, 0, 3)])]


def rank_dict(words):
    """word -> rank; of a duplicate word the first wins, the empty word has none"""
    d = {}
    for i, w in enumerate(words):
        if len(w):
            d.setdefault(bytes(w), i)
    return d


def cut(token, d, max_bytes=4096, unk=-1, ids=None):
    """the pieces of one token (non-empty bytes): [(id, start, end)], byte positions inside the token; also returns nothing else.
    ``d``: rank_dict of the words; ``ids``: the optional id of every rank"""
    token = bytes(token)
    ident = (lambda r: r) if ids is None else (lambda r: int(ids[r]))
    if len(token) > max_bytes:
        return [(unk, 0, len(token))]
    if token in d:
        return [(ident(d[token]), 0, len(token))]
    parts = [token[i:i + 1] for i in range(len(token))]
    while True:
        best = None
        for i in range(len(parts) - 1):
            r = d.get(parts[i] + parts[i + 1])
            if r is not None and (best is None or r < best[0]):      # (strictly lower: of equal ranks the leftmost stays)
                best = (r, i)
        if best is None:
            break
        parts[best[1]:best[1] + 2] = [parts[best[1]] + parts[best[1] + 1]]
    out, at = [], 0
    for p in parts:
        out.append((ident(d[p]) if p in d else unk, at, at + len(p)))
        at += len(p)
    return out


def merges(token, d, max_bytes=4096):
    """how many merges cut() makes for the token (0 for the two one-piece outcomes)"""
    token = bytes(token)
    if len(token) > max_bytes or token in d:
        return 0
    return len(token) - len(cut(token, d, max_bytes))


def cut_rows(utf8, byte_off, counts, spans, d, max_bytes=4096, lead_space=False, unk=-1, ids=None):
    """a batch: utf8 / byte_off as the calls take them, counts / spans as token_spans_utf8_bytes_csr returns them ->
    (indptr list, ids list, piece spans list of (start, end) relative to the string)"""
    data = bytes(bytearray(utf8))
    indptr, out_ids, out_spans, k = [0], [], [], 0
    for s in range(len(byte_off) - 1):
        base = int(byte_off[s])
        for _ in range(int(counts[s])):
            a, e = int(spans[k][0]), int(spans[k][1])
            k += 1
            if lead_space and a > 0 and data[base + a - 1] == 0x20:
                a -= 1
            for pid, p0, p1 in cut(data[base + a:base + e], d, max_bytes, unk, ids):
                out_ids.append(pid)
                out_spans.append((a + p0, a + p1))
        indptr.append(len(out_ids))
    return indptr, out_ids, out_spans


def train(corpus_tokens, n_merges, base=None):
    """A tiny byte-pair trainer: the words are the single bytes in `base` (default: every byte that occurs, ascending), then
    n_merges times the most frequent adjacent pair of the corpus (ties: the lowest bytes), merged everywhere.  corpus_tokens: an
    iterable of bytes.  Returns the list of words in rank order."""
    freq = Counter(bytes(t) for t in corpus_tokens)
    seqs = {t: [t[i:i + 1] for i in range(len(t))] for t in freq}
    words = [bytes([b]) for b in (sorted({b for t in freq for b in t}) if base is None else base)]
    for _ in range(n_merges):
        pairs = Counter()
        for t, parts in seqs.items():
            for i in range(len(parts) - 1):
                pairs[(parts[i], parts[i + 1])] += freq[t]
        if not pairs:
            break
        (x, y), _n = min(pairs.items(), key=lambda kv: (-kv[1], kv[0]))
        words.append(x + y)
        for t, parts in seqs.items():
            i, out = 0, []
            while i < len(parts):
                if i + 1 < len(parts) and parts[i] == x and parts[i + 1] == y:
                    out.append(x + y)
                    i += 2
                else:
                    out.append(parts[i])
                    i += 1
            seqs[t] = out
    return words
