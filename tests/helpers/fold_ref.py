"""The definition of latok_fold_utf8_bytes_batch (include/latok_hip.h) restated in plain Python over BYTES, twice: a scalar walk
that is meant to be obviously right (``fold_bytes``) and a numpy form for batches of several MB (``fold_batch``).  The per-code-point
map F_fold is read from tests/golden/fold_map.json (tests/golden/make_fold_golden.py) plus the Hangul arithmetic and the CJK ranges.

* per string: a byte b0 at i with k = n_cont(b0) > 0 opens a SEQUENCE iff bytes i+1 .. i+k lie inside the same string and are all
  10xxxxxx; a byte below 0x80 is a sequence of its own; the value is the payload as utf8_ref.cp_at puts it together;
* a sequence whose image is [c] is copied verbatim, any other is replaced by the shortest-form UTF-8 of its image;
* every byte that belongs to no sequence is copied verbatim; fold == 0 copies everything.

Nothing here is derived from the code under test."""
import json
import os

import numpy as np

LOWER, STRIP_MARKS, CLEAN, CJK_SPACE = 1, 2, 4, 8
UNCASED, ALL = LOWER | STRIP_MARKS, 15
COMBOS = (0, LOWER, STRIP_MARKS, CLEAN, CJK_SPACE, LOWER | STRIP_MARKS, ALL)
S_BASE, L_BASE, V_BASE, T_BASE, S_COUNT, N_COUNT, T_COUNT = 0xAC00, 0x1100, 0x1161, 0x11A7, 11172, 588, 28
CJK_RANGES = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F), (0x2B820, 0x2CEAF),
              (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))
N_CP = 0x110000

_G = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "golden", "fold_map.json")))
UNIDATA_VERSION = _G["unidata_version"]
LOWER_OF = {c: lo for c, lo, _ in _G["map"]}
STRIP_OF = {c: st for c, _, st in _G["map"]}
CC_CF = frozenset(c for a, b in _G["cc_cf"] for c in range(a, b + 1))
ZS = frozenset(c for a, b in _G["zs"] for c in range(a, b + 1))


def n_cont(b0):
    return 0 if b0 < 0xC0 else 1 if b0 < 0xE0 else 2 if b0 < 0xF0 else 3


def is_cjk(c):
    return any(a <= c <= b for a, b in CJK_RANGES)


def strip_cp(x):
    if S_BASE <= x < S_BASE + S_COUNT:
        s = x - S_BASE
        out = [L_BASE + s // N_COUNT, V_BASE + (s % N_COUNT) // T_COUNT]
        return out + [T_BASE + s % T_COUNT] if s % T_COUNT else out
    return STRIP_OF.get(x, [x])


def fold_cp(c, fold):
    """F_fold(c): the list of code points"""
    if fold == 0 or 0xD800 <= c <= 0xDFFF or c > 0x10FFFF:
        return [c]
    if fold & CLEAN:
        if c in (9, 10, 13, 0x20) or c in ZS:
            return [0x20]
        if c == 0 or c == 0xFFFD or c in CC_CF:
            return []
    seq = [c]
    if fold & LOWER:
        seq = list(LOWER_OF.get(c, [c]))
    if fold & STRIP_MARKS:
        seq = [y for x in seq for y in strip_cp(x)]
    if fold & CJK_SPACE and is_cjk(c):
        seq = [0x20] + seq + [0x20]
    return seq


def encode(seq):
    return "".join(map(chr, seq)).encode("utf-8", "surrogatepass")


def fold_bytes(data, fold):
    """one string, the scalar walk"""
    data = bytes(data)
    out, i, n = bytearray(), 0, len(data)
    while i < n:
        b0 = data[i]
        k = n_cont(b0)
        if b0 >= 0x80 and (k == 0 or i + k >= n or any((b & 0xC0) != 0x80 for b in data[i + 1:i + 1 + k])):
            out.append(b0)                       # no sequence: the byte itself
            i += 1
            continue
        c = b0 if k == 0 else b0 & (0x3F >> k)
        for b in data[i + 1:i + 1 + k]:
            c = (c << 6) | (b & 0x3F)
        img = fold_cp(c, fold)
        out += data[i:i + 1 + k] if img == [c] else encode(img)
        i += 1 + k
    return bytes(out)


def fold_blobs(blobs, fold):
    return [fold_bytes(b, fold) for b in blobs]


def fold_batch_scalar(u8, byte_off, fold):
    u8, off = bytes(np.asarray(u8, np.uint8)), [int(o) for o in byte_off]
    rows = [fold_bytes(u8[off[s]:off[s + 1]], fold) for s in range(len(off) - 1)]
    out_off = np.zeros(len(off), np.int64)
    out_off[1:] = np.cumsum([len(r) for r in rows])
    return np.frombuffer(b"".join(rows), np.uint8), out_off


# ---- the numpy form ----------------------------------------------------------------------------------------------------------
_DENSE = {}


def dense(fold):
    """(n uint8[N_CP + 1], cps uint32[N_CP + 1, 3]): F_fold of every code point; entry N_CP stands for every value above 0x10FFFF"""
    if fold not in _DENSE:
        n = np.ones(N_CP + 1, np.uint8)
        cps = np.zeros((N_CP + 1, 3), np.uint32)
        cps[:, 0] = np.arange(N_CP + 1)
        special = set(LOWER_OF) | set(range(S_BASE, S_BASE + S_COUNT)) | CC_CF | ZS | {0, 9, 10, 13, 0x20, 0xFFFD}
        if fold & CJK_SPACE:
            special |= {c for a, b in CJK_RANGES for c in range(a, b + 1)}
        for c in (special if fold else ()):
            img = fold_cp(c, fold)
            n[c] = len(img)
            cps[c, :] = 0
            cps[c, :len(img)] = img
        _DENSE[fold] = (n, cps)
    return _DENSE[fold]


def _enc(cp):
    """uint32[U] -> (bytes uint8[U, 4], len uint8[U]): shortest-form UTF-8"""
    cp = cp.astype(np.uint32)
    ln = 1 + (cp >= 0x80).astype(np.uint8) + (cp >= 0x800) + (cp >= 0x10000)
    b = np.zeros((cp.size, 4), np.uint8)
    for L, lead in ((1, 0x00), (2, 0xC0), (3, 0xE0), (4, 0xF0)):
        m = ln == L
        x = cp[m]
        for j in range(L):
            sh = 6 * (L - 1 - j)
            b[m, j] = ((x >> sh) & (0x7F if L == 1 else 0x3F if j else 0xFF)) | (0x80 if j else lead)
    return b, ln


def fold_batch(u8, byte_off, fold):
    """(out uint8[n], out_off int64[n_str + 1]) of a packed batch"""
    u8 = np.ascontiguousarray(u8, np.uint8)
    byte_off = np.asarray(byte_off, np.int64)
    total = int(byte_off[-1]) if byte_off.size else 0
    u8 = u8[:total]
    if total == 0:
        return np.zeros(0, np.uint8), np.zeros(byte_off.size, np.int64)
    pos = np.arange(total, dtype=np.int64)
    end = byte_off[np.searchsorted(byte_off, pos, side="right")]              # the end of the string that holds each byte
    pad = np.concatenate([u8, np.zeros(3, np.uint8)])
    b0 = u8.astype(np.uint32)
    k = (b0 >= 0xC0).astype(np.int64) + (b0 >= 0xE0) + (b0 >= 0xF0)
    seq = (k > 0) & (pos + k < end)
    cp = np.where(k > 0, b0 & (np.uint32(0x3F) >> k.astype(np.uint32)), b0)
    for j in (1, 2, 3):
        nxt = pad[pos + j].astype(np.uint32)
        need = k >= j
        seq &= ~need | ((nxt & 0xC0) == 0x80)
        cp = np.where(need, (cp << np.uint32(6)) | (nxt & 0x3F), cp)
    consumed = np.zeros(total + 3, bool)
    for j in (1, 2, 3):
        consumed[pos[seq & (k >= j)] + j] = True
    consumed = consumed[:total]
    char = (seq | (b0 < 0x80)) & ~consumed                                    # sequences, ASCII included
    raw = ~char & ~consumed                                                   # bytes of no sequence
    n_img, img = dense(fold)
    idx = np.minimum(cp, N_CP).astype(np.int64)
    n_c = np.where(char, n_img[idx], 0)
    same = char & (n_c == 1) & (img[idx, 0] == cp)
    verb = raw | same
    units = np.flatnonzero(verb | char)
    U = units.size
    cell = np.zeros((U, 12), np.uint8)
    keep = np.zeros((U, 12), bool)
    v = verb[units]
    for j in range(4):                                                        # verbatim: the source bytes
        cell[v, j] = pad[units[v] + j]
        keep[v, j] = j <= np.where(raw[units[v]], 0, k[units[v]])
    e = ~v
    for s in range(3):
        rows = e & (n_c[units] > s)
        b, ln = _enc(img[idx[units[rows]], s])
        cell[rows, 4 * s:4 * s + 4] = b
        keep[rows, 4 * s:4 * s + 4] = np.arange(4)[None, :] < ln[:, None]
    out = cell[keep]
    per_byte = np.zeros(total + 1, np.int64)
    per_byte[units + 1] = keep.sum(axis=1)
    return out, np.cumsum(per_byte)[np.clip(byte_off, 0, total)]
