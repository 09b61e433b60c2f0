"""A token with a chosen MurmurHash3 x86_32 hash: what makes the h = -2^31 rule of the hashed term counts testable.

Every step of the function behind the last block is invertible: fmix32 is two multiplications by odd constants and three
xor-shifts, the length xor undoes itself, and a block step (a rotation, a multiplication by 5, an addition) can be solved for the
block.  So for an 8-byte token -- two blocks, no tail -- the FIRST block is free and the second one follows from it:

    h2 = unfmix32(target) ^ 8;  h1 = mix_h(seed, mix_k(block0));  block1 = unmix_k(rotr((h2 - N) / 5, 13) ^ h1)

``token_with_hash`` searches the free block over an alphabet until all eight bytes lie in it -- no byte is whitespace, and with
the default alphabet (lower-case letters) no rule of the tokenizer cuts the token."""
import itertools

from helpers.murmur3_collide import FIVE_INV, M, N, _rotr, mix_h, mix_k, unmix_k
from helpers.murmur3_ref import murmur3_ref

F1_INV, F2_INV = pow(0x85EBCA6B, -1, 1 << 32), pow(0xC2B2AE35, -1, 1 << 32)


def _unxorshift(h, s):
    x = h
    for _ in range(32 // s + 1):
        x = h ^ (x >> s)
    return x


def unfmix32(h):
    h = _unxorshift(h, 16)
    h = h * F2_INV & M
    h = _unxorshift(h, 13)
    h = h * F1_INV & M
    return _unxorshift(h, 16)


def token_with_hash(target, seed=0, alphabet=b"abcdefghijklmnopqrstuvwxyz"):
    """8 bytes of ``alphabet`` whose hash with ``seed`` is ``target`` (an unsigned 32-bit value)"""
    ok = set(alphabet)
    h2 = unfmix32(target & M) ^ 8
    want = _rotr((h2 - N) * FIVE_INV & M, 13)          # h1 ^ mix_k(block1)
    for first in itertools.product(alphabet, repeat=4):
        h1 = mix_h(seed, mix_k(int.from_bytes(bytes(first), "little")))
        second = unmix_k(want ^ h1).to_bytes(4, "little")
        if all(b in ok for b in second):
            tok = bytes(first) + second
            assert murmur3_ref(tok, seed) == target & M
            return tok
    raise AssertionError("no token over this alphabet")


INT32_MIN_TOKEN = b"akqlrggi"      # token_with_hash(0x80000000, 0): the hash is -2^31 as int32 under seed 0
