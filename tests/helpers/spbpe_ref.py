"""SentencePiece BPE, restated from the definition in include/latok_hip.h (behind latok_bpe_create_spm) over ``bytes`` and one ``dict``:
the reference the host harness of spbpe.h and the device calls are held to.  It shares no code and no data structure with either: a
list of characters, a list of parts rescanned whole in every round, and one list that says which real bytes every virtual character
stands for."""
MARK = b"\xe2\x96\x81"   # U+2581


def chars(data):
    """the characters of one range of bytes: [(start, end)]; a character starts at the first byte and at every byte that is not 10xxxxxx"""
    out, i, n = [], 0, len(data)
    while i < n:
        e = i + 1
        while e < n and (data[e] & 0xC0) == 0x80:
            e += 1
        out.append((i, e))
        i = e
    return out


def space_like(c):
    return c == b" " or c == MARK


def segments(data):
    """the segments of one string: [(start, end)].  An empty string has none."""
    data = bytes(data)
    starts, prev = [], False
    for a, e in chars(data):
        sl = space_like(data[a:e])
        if a == 0 or (sl and not prev):
            starts.append(a)
        prev = sl
    return list(zip(starts, starts[1:] + [len(data)]))


def virtual(seg, dummy):
    """the virtual text of one segment as a list of (character bytes, real start, real end), positions inside the segment"""
    out = [(MARK, 0, 0)] if dummy else []
    lead = True
    for a, e in chars(seg):
        c = seg[a:e]
        lead = lead and space_like(c)
        out.append((MARK if lead else c, a, e))
    return out


def cut(seg, d, first=True, byte_ids=None, add_dummy_prefix=True, fuse_unk=False, max_bytes=4096, unk=-1, ids=None):
    """the pieces of one segment (non-empty bytes): [(id, start, end)], real byte positions inside the segment.  ``d``: word -> rank (of a
    duplicate the first wins); ``ids``: the optional id of every rank; ``first``: the segment is its string's first"""
    seg = bytes(seg)
    ident = (lambda r: r) if ids is None else (lambda r: int(ids[r]))
    v = virtual(seg, bool(add_dummy_prefix) and first)
    if sum(len(c) for c, _, _ in v) > max_bytes:
        return [(unk, 0, len(seg))]
    parts = [(c, a, e, 1) for c, a, e in v]        # bytes, real start, real end, characters
    while True:
        best = None
        for i in range(len(parts) - 1):
            r = d.get(parts[i][0] + parts[i + 1][0])
            if r is not None and (best is None or r < best[0]):   # (strictly lower: of equal ranks the leftmost stays)
                best = (r, i)
        if best is None:
            break
        i = best[1]
        x, y = parts[i], parts[i + 1]
        parts[i:i + 2] = [(x[0] + y[0], x[1], y[2], x[3] + y[3])]
    out, run = [], False
    for c, a, e, n in parts:
        if c in d:
            out.append((ident(d[c]), a, e))
            run = False
            continue
        assert n == 1                               # (every merged part is a word)
        if byte_ids is not None:
            out.extend((int(byte_ids[b]), a, e) for b in c)
        elif fuse_unk and run:
            out[-1] = (unk, out[-1][1], e)
        else:
            out.append((unk, a, e))
            run = True
    return out


def rank_dict(words):
    d = {}
    for i, w in enumerate(words):
        if len(w):
            d.setdefault(bytes(w), i)
    return d


def encode(text, d, **kw):
    """one string (bytes) -> (ids, spans relative to the string)"""
    text = bytes(text)
    out_ids, out_spans = [], []
    for a, e in segments(text):
        for pid, p0, p1 in cut(text[a:e], d, first=(a == 0), **kw):
            out_ids.append(pid)
            out_spans.append((a + p0, a + p1))
    return out_ids, out_spans


def encode_rows(texts, d, **kw):
    """a batch -> (indptr, ids, spans)"""
    indptr, out_ids, out_spans = [0], [], []
    for t in texts:
        i, s = encode(t, d, **kw)
        out_ids += i
        out_spans += s
        indptr.append(len(out_ids))
    return indptr, out_ids, out_spans


def bad_word(words):
    """the position of the first word that holds the marker directly behind a character that is not the marker, or -1"""
    for w, word in enumerate(words):
        prev = True
        for a, e in chars(bytes(word)):
            m = bytes(word)[a:e] == MARK
            if m and not prev:
                return w
            prev = m
    return -1
