"""Decoding, restated plainly (include/latok_hip.h: latok_detok_*): ids back to bytes over Python lists and a dict.  The reference of
tests/test_detok_host.py (against detok.h under g++) and tests/test_gpu_detok.py (against the device)."""

CONCAT, WORDPIECE = 0, 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def id_map(words, ids=None):
    """id -> word; of several words with one id the lowest index wins"""
    d = {}
    for i, w in enumerate(words):
        d.setdefault(i if ids is None else ids[i], w)
    return d


def is_continuation(word, prefix):
    return word.startswith(prefix) and len(word) > len(prefix)


def decode_row(row, d, mode=CONCAT, prefix=b"##", sep=b" ", skip=()):
    """(bytes of the row, unknown ids in it)"""
    out, kept, unknown = [], 0, 0
    for i in row:
        if i in skip:
            continue
        if i not in d:
            unknown += 1
            continue
        w = d[i]
        if mode == CONCAT or kept == 0:
            out.append(w)
        elif is_continuation(w, prefix):
            out.append(w[len(prefix):])
        else:
            out.append(sep + w)
        kept += 1
    return b"".join(out), unknown


def decode(rows, d, mode=CONCAT, prefix=b"##", sep=b" ", skip=()):
    """(list of the rows' bytes, unknown ids of the batch)"""
    got = [decode_row(r, d, mode, prefix, sep, skip) for r in rows]
    return [g[0] for g in got], sum(g[1] for g in got)


def padded_rows(block, lengths=None):
    """the rows of a padded [n, L] block: the first lengths[s] cells of row s (all of them without lengths)"""
    return [list(r[:len(r) if lengths is None else lengths[s]]) for s, r in enumerate(block)]


def is_dense(words, ids, spread):
    """the form the object takes: dense iff the id range is at most `spread` times the word count"""
    n = len(words)
    if n == 0:
        return False
    ids = list(range(n)) if ids is None else ids
    return max(ids) - min(ids) + 1 <= spread * n


def join_replace(row_words, prefix=b"##", sep=b" "):
    """the rule of BERT tokenizers: sep.join(words).replace(sep + prefix, b"")"""
    return sep.join(row_words).replace(sep + prefix, b"")
