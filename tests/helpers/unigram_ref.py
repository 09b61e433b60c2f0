"""The Unigram cut, restated from the definition in include/latok_hip.h over ``bytes``, one ``dict`` and ``numpy.float32``: the
reference the host harness of unigram.h and the device calls are held to.  It shares no code and no data structure with either: the
virtual text is built, its positions are a list, every slice is looked up in the dict."""
import numpy as np

MARKER = "▁".encode()


def word_dict(words):
    """word -> position; of a duplicate word the first wins, the empty word has none"""
    d = {}
    for i, w in enumerate(words):
        if len(w):
            d.setdefault(bytes(w), i)
    return d


def default_unk_score(scores):
    """SentencePiece's penalty: float32(min(scores)) - 10"""
    return np.float32(min(np.float32(s) for s in scores)) - np.float32(10) if len(scores) else np.float32(-10)


def positions(text):
    """the character starts of a byte range, plus its end"""
    return [i for i in range(len(text)) if i == 0 or (text[i] & 0xC0) != 0x80] + [len(text)]


def cut(token, marked, d, scores, unk_score, marker=MARKER, fuse_unk=True, max_bytes=4096, unk=-1, ids=None):
    """the pieces of one token (non-empty bytes): [(id, start, end)], byte positions inside the token.  ``marked``: the token takes
    the marker (ignored when the marker is empty); ``d``: word_dict of the words; ``scores``: one per word; ``ids``: optional, one per word"""
    token = bytes(token)
    ident = (lambda w: w) if ids is None else (lambda w: int(ids[w]))
    if len(token) > max_bytes:
        return [(unk, 0, len(token))]
    m = len(marker) if marked and len(marker) else 0
    text = (bytes(marker) if m else b"") + token
    pos = positions(text)
    n = len(pos) - 1
    best = [None] * (n + 1)
    back = [None] * (n + 1)
    best[0] = np.float32(0.0)
    unk_score = np.float32(unk_score)
    for i in range(n):
        if best[i] is None:
            continue
        single = False
        for j in range(i + 1, n + 1):
            w = d.get(text[pos[i]:pos[j]])
            if w is None:
                continue
            single = single or j == i + 1
            cand = np.float32(best[i] + np.float32(scores[w]))
            if best[j] is None or cand > best[j]:
                best[j], back[j] = cand, (i, w)
        if not single:
            cand = np.float32(best[i] + unk_score)
            if best[i + 1] is None or cand > best[i + 1]:
                best[i + 1], back[i + 1] = cand, (i, None)
    assert all(b is not None for b in best)
    pieces, j = [], n
    while j > 0:
        i, w = back[j]
        pieces.append((w, max(pos[i] - m, 0), pos[j] - m))
        j = i
    pieces.reverse()
    out = []
    for w, s, e in pieces:
        if w is None and fuse_unk and out and out[-1][0] is None:
            out[-1] = (None, out[-1][1], e)
        else:
            out.append((w, s, e))
    return [(unk if w is None else ident(w), s, e) for w, s, e in out]


def is_marked(prev_end, start):
    """a token of a string: prev_end = the end of the token before it in the same string, None for the first"""
    return prev_end is None or prev_end < start


def cut_rows(utf8, byte_off, counts, spans, d, scores, unk_score, marker=MARKER, fuse_unk=True, max_bytes=4096, unk=-1, ids=None):
    """a batch: utf8 / byte_off as the calls take them, counts / spans as token_spans_utf8_bytes_csr returns them ->
    (indptr, ids, spans): the pieces of every string, spans string-relative"""
    data = bytes(np.asarray(utf8, np.uint8))
    indptr, out_ids, out_spans, t = [0], [], [], 0
    for s, c in enumerate(counts):
        base, prev = int(byte_off[s]), None
        for _ in range(int(c)):
            a, e = int(spans[t][0]), int(spans[t][1])
            for pid, ps, pe in cut(data[base + a:base + e], is_marked(prev, a), d, scores, unk_score, marker, fuse_unk, max_bytes, unk, ids):
                out_ids.append(pid)
                out_spans.append((a + ps, a + pe))
            prev = e
            t += 1
        indptr.append(len(out_ids))
    return (np.array(indptr, np.int64), np.array(out_ids, np.int32).reshape(-1), np.array(out_spans, np.int64).reshape(-1, 2))
