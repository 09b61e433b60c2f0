"""WordPiece, restated from the definition in include/latok_hip.h over ``bytes`` and one ``dict``: the reference the host harness
of wordpiece.h and the device calls are held to.  It shares no code and no data structure with either: one dictionary that is
asked for ``piece`` at a token's start and for ``prefix + piece`` elsewhere."""


def vocab_dict(words, ids=None):
    """word -> id; of a duplicate word the first wins"""
    d = {}
    for i, w in enumerate(words):
        d.setdefault(bytes(w), i if ids is None else int(ids[i]))
    return d


def is_char_start(token, i):
    return i == 0 or (token[i] & 0xC0) != 0x80


def chars(token):
    return sum(is_char_start(token, i) for i in range(len(token)))


def cut(token, d, prefix=b"##", max_chars=100, unk=-1):
    """the pieces of one token (non-empty bytes): [(id, start, end)], byte positions inside the token"""
    n = len(token)
    if chars(token) > max_chars:
        return [(unk, 0, n)]
    out, start = [], 0
    while start < n:
        for p in range(n, start, -1):
            if p != n and not is_char_start(token, p):
                continue
            key = token[start:p] if start == 0 else prefix + token[start:p]
            if key in d:
                out.append((d[key], start, p))
                break
        else:
            return [(unk, 0, n)]
        start = p
    return out


def cut_rows(utf8, byte_off, counts, spans, d, prefix=b"##", max_chars=100, unk=-1):
    """a batch: utf8 / byte_off as the calls take them, counts / spans as token_spans_utf8_bytes_csr returns them ->
    (indptr list, ids list, piece spans list of (start, end) relative to the string)"""
    data = bytes(bytearray(utf8))
    indptr, ids, out_spans, k = [0], [], [], 0
    for s in range(len(byte_off) - 1):
        base = int(byte_off[s])
        for _ in range(int(counts[s])):
            a, e = int(spans[k][0]), int(spans[k][1])
            k += 1
            for pid, p0, p1 in cut(data[base + a:base + e], d, prefix, max_chars, unk):
                ids.append(pid)
                out_spans.append((a + p0, a + p1))
        indptr.append(len(ids))
    return indptr, ids, out_spans
