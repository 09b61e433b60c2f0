"""Crafted MurmurHash3 x86_32 collisions: what makes the byte compare of the vocabulary lookup testable.

The block steps of the function are invertible (a multiplication by an odd constant, a rotation, an xor), so for a byte string
``a`` one can change one block and SOLVE the next one for the internal state to meet again:

  block pair   ``a`` differs from ``b`` in block i (one changed byte) and in block i + 1 (solved).  Needs i + 1 < len(a) // 4.
  tail         ``b`` differs in the tail (one changed byte of the 1..3 bytes behind the last whole block) and in the last whole
               block (solved).  Needs len(a) >= 5 and len(a) % 4 != 0.

Both give len(b) == len(a), b != a and murmur3(b, seed) == murmur3(a, seed).  Strings of 1 to 4 bytes cannot collide at equal
length: the function is injective there.  Candidates are tried until the first and the last byte of ``b`` are non-whitespace
ASCII (0x21 .. 0x7e), so that a tokenizer that strips whitespace at both ends leaves ``b`` whole; the bytes in between are
whatever the solution asks for.  ``word_pairs`` repeats a numpy search that finds colliding pairs of plain 8-letter words."""
import numpy as np

from helpers.murmur3_ref import murmur3_ref

M = 0xFFFFFFFF
C1, C2, N = 0xCC9E2D51, 0x1B873593, 0xE6546B64
C1_INV, C2_INV, FIVE_INV = pow(C1, -1, 1 << 32), pow(C2, -1, 1 << 32), pow(5, -1, 1 << 32)


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M


def _rotr(x, r):
    return ((x >> r) | (x << (32 - r))) & M


def mix_k(k):
    return _rotl(k * C1 & M, 15) * C2 & M


def unmix_k(m):
    return _rotr(m * C2_INV & M, 15) * C1_INV & M


def mix_h(h, mk):
    return (_rotl(h ^ mk, 13) * 5 + N) & M


def _state(data, seed, n_blocks):
    """the internal state behind the first n_blocks blocks"""
    h = seed
    for i in range(n_blocks):
        h = mix_h(h, mix_k(int.from_bytes(data[4 * i:4 * i + 4], "little")))
    return h


def _printable_ends(b):
    return 0x21 <= b[0] <= 0x7E and 0x21 <= b[-1] <= 0x7E


def _changes():
    """(byte of the block / tail, new-value xor) in a fixed order"""
    for x in range(1, 256):
        for pos in range(4):
            yield pos, x


def collide_blocks(a, seed, i):
    """``b``: as long as ``a``, the same hash, other bytes in blocks i and i + 1 only"""
    a = bytes(a)
    assert 0 <= i and i + 1 < len(a) // 4, (len(a), i)
    h_before = _state(a, seed, i)
    h_a = mix_h(h_before, mix_k(int.from_bytes(a[4 * i:4 * i + 4], "little")))
    mk_next = mix_k(int.from_bytes(a[4 * i + 4:4 * i + 8], "little"))
    for pos, x in _changes():
        blk = bytearray(a[4 * i:4 * i + 4])
        blk[pos] ^= x
        h_b = mix_h(h_before, mix_k(int.from_bytes(blk, "little")))
        nxt = unmix_k(mk_next ^ h_a ^ h_b)             # h_b ^ mix_k(nxt) == h_a ^ mk_next: the states meet behind block i + 1
        b = a[:4 * i] + bytes(blk) + nxt.to_bytes(4, "little") + a[4 * i + 8:]
        if _printable_ends(b):
            assert b != a and len(b) == len(a) and murmur3_ref(b, seed) == murmur3_ref(a, seed)
            assert [j for j in range(len(a)) if a[j] != b[j]][0] // 4 == i and [j for j in range(len(a)) if a[j] != b[j]][-1] // 4 == i + 1
            return b
    raise AssertionError("no candidate with printable ends")


def collide_tail(a, seed):
    """``b``: as long as ``a``, the same hash, other bytes in the tail and in the last whole block only"""
    a = bytes(a)
    nb, t = len(a) // 4, len(a) % 4
    assert nb >= 1 and t, len(a)
    h_prev = _state(a, seed, nb - 1)
    h_a = mix_h(h_prev, mix_k(int.from_bytes(a[4 * nb - 4:4 * nb], "little")))
    mk_tail = mix_k(int.from_bytes(a[4 * nb:], "little"))
    for pos, x in _changes():
        if pos >= t:
            continue
        tail = bytearray(a[4 * nb:])
        tail[pos] ^= x
        want = h_a ^ mk_tail ^ mix_k(int.from_bytes(tail, "little"))      # the state the last whole block must leave
        blk = unmix_k(_rotr((want - N) * FIVE_INV & M, 13) ^ h_prev)
        b = a[:4 * nb - 4] + blk.to_bytes(4, "little") + bytes(tail)
        if _printable_ends(b) and b[:4 * nb] != a[:4 * nb]:
            assert b != a and len(b) == len(a) and murmur3_ref(b, seed) == murmur3_ref(a, seed)
            return b
    raise AssertionError("no candidate with printable ends")


def positions(n):
    """every place collide() offers for a string of n bytes: block indices i (pair i, i + 1) and "tail\""""
    out = list(range(0, n // 4 - 1))
    if n >= 5 and n % 4:
        out.append("tail")
    return out


def collide(a, seed, where):
    return collide_tail(a, seed) if where == "tail" else collide_blocks(a, seed, where)


def word_pairs(seed=0, want=2, letters=b"abcdefghijklmnopqrstuvwxyz", rng_seed=1, n=1 << 21):
    """pairs of distinct 8-letter words (4 random letters + 'aaaa' / 'baaa' tails are enough) with one hash: a birthday search
    over n random words, vectorised.  Returns at most ``want`` pairs of bytes."""
    rng = np.random.default_rng(rng_seed)
    words = np.frombuffer(bytes(letters), np.uint8)[rng.integers(0, len(letters), (n, 8))]
    words[:, 5:] = ord("a")
    words[:, 4] = np.where(rng.integers(0, 2, n) == 1, ord("b"), ord("a"))
    words = np.unique(np.ascontiguousarray(words).view("<u8").ravel()).view(np.uint8).reshape(-1, 8)
    k = words.view("<u4").astype(np.uint64)

    def rotl(x, r):
        return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & np.uint64(M)

    h = np.full(len(words), seed, np.uint64)
    for j in range(2):
        mk = rotl(k[:, j] * np.uint64(C1) & np.uint64(M), 15) * np.uint64(C2) & np.uint64(M)
        h = (rotl(h ^ mk, 13) * np.uint64(5) + np.uint64(N)) & np.uint64(M)
    h ^= np.uint64(8)
    h = (h ^ (h >> np.uint64(16))) * np.uint64(0x85EBCA6B) & np.uint64(M)
    h = (h ^ (h >> np.uint64(13))) * np.uint64(0xC2B2AE35) & np.uint64(M)
    h ^= h >> np.uint64(16)
    order = np.argsort(h, kind="stable")
    hs = h[order]
    hit = np.nonzero(hs[1:] == hs[:-1])[0]
    pairs = []
    for j in hit[:want]:
        a, b = words[order[j]].tobytes(), words[order[j + 1]].tobytes()
        assert a != b and murmur3_ref(a, seed) == murmur3_ref(b, seed)
        pairs.append((a, b))
    return pairs


KNOWN_WORD_PAIRS = ((b"qkjlaaaa", b"idugbaaa"), (b"kijjaaaa", b"cbuebaaa"))      # seed 0
