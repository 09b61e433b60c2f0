"""MurmurHash3 x86_32 in plain Python, written for the tests (independent of latok_amd.batch.murmur3_32 and of token_hash.h): the
host reference the device's token hashes are compared with.  VECTORS are the published test vectors of the function."""
import struct

MASK = 0xFFFFFFFF
C1, C2 = 0xCC9E2D51, 0x1B873593

VECTORS = [
    (b"", 0, 0x00000000), (b"", 1, 0x514E28B7), (b"", 0xFFFFFFFF, 0x81F16F39),
    (b"test", 0, 0xBA6BD213), (b"test", 0x9747B28C, 0x704B81DC),
    (b"Hello, world!", 0, 0xC0363E43), (b"Hello, world!", 0x9747B28C, 0x24884CBA),
    (b"The quick brown fox jumps over the lazy dog", 0, 0x2E4FF723),
    (b"The quick brown fox jumps over the lazy dog", 0x9747B28C, 0x2FA826CD),
    (b"a", 0, 0x3C2569B2), (b"ab", 0, 0x9BBFD75F), (b"abc", 0, 0xB3DD93FA), (b"abcd", 0, 0x43ED676A), (b"abcde", 0, 0xE89B9AF6),
]
SEEDS = (0, 1, 0x9747B28C, 0xFFFFFFFF)


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & MASK


def murmur3_ref(data, seed=0):
    data = bytes(data)
    n = len(data)
    h = seed & MASK
    n_blocks = n // 4
    for k in struct.unpack_from("<%dI" % n_blocks, data):
        k = (k * C1) & MASK
        k = (_rotl(k, 15) * C2) & MASK
        h = (_rotl(h ^ k, 13) * 5 + 0xE6546B64) & MASK
    tail = data[4 * n_blocks:]
    if tail:
        k = 0
        for i in reversed(range(len(tail))):
            k = (k << 8) | tail[i]
        k = (k * C1) & MASK
        k = (_rotl(k, 15) * C2) & MASK
        h ^= k
    h ^= n & MASK
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & MASK
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & MASK
    h ^= h >> 16
    return h
