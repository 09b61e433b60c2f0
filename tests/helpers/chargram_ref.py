"""Character n-grams inside tokens (include/latok_hip.h: latok_chargram_counts_utf8_bytes_batch), restated in plain Python from the
definition alone: list slicing over a token's characters, nothing shared with latok_amd/csrc/chargram_text.h.  The hash of a gram is
helpers.murmur3_ref.murmur3_ref of its bytes."""
RANGES = [(1, 1), (1, 2), (2, 2), (3, 5), (4, 4), (2, 8), (8, 8), (1, 8)]
# tokens of malformed bytes: a continuation byte first, runs of them, a truncated lead as the last byte, 0xC0 and 0xF8 .. 0xFF
MALFORMED = [b"\x80abc", b"\x80\x81\x82", b"\xbf\xbf\xbf\xbfx\x80\x80", b"ab\xe2", b"ab\xe2\x82", b"\xf0", b"\xc0\xaf", b"\xc0", b"a\xf8\x88\x80\x80\x80b",
             b"\xf9\xfa\xfb", b"\xfc\xfd\xfe\xff", b"\xff", b"x\xfey\xffz", b"\x80", b"\xe6\x97\xa5\x80\x80\xe6", b"\xf8\x80" * 5]


def chars_of(token: bytes):
    """the token's characters: one starts at the first byte and at every later byte that is no continuation byte"""
    starts = [0] + [k for k in range(1, len(token)) if (token[k] & 0xC0) != 0x80]
    return [token[a:b] for a, b in zip(starts, starts[1:] + [len(token)])]


def padded_word(token: bytes, pad: int = 0x20):
    return [bytes([pad])] + chars_of(token) + [bytes([pad])]


def token_grams(token: bytes, min_n: int, max_n: int, pad: int = 0x20):
    """[(n, i, gram bytes)] in the definition's order: orders ascending, start positions ascending; a padded word of W <= n characters
    gives the whole word once and no higher order contributes.  An empty token has no gram."""
    if not token:
        return []
    w = padded_word(token, pad)
    out = []
    for n in range(min_n, max_n + 1):
        if n < len(w):
            out += [(n, i, b"".join(w[i:i + n])) for i in range(len(w) - n + 1)]
        else:
            out.append((n, 0, b"".join(w)))
            break
    return out


def gram_count(n_chars: int, min_n: int, max_n: int) -> int:
    """G(W) of the header, W = n_chars + 2"""
    w = n_chars + 2
    return sum(w - n + 1 for n in range(min_n, min(max_n, w - 1) + 1)) + (1 if max_n >= w else 0)


def token_slots(token: bytes, min_n: int, max_n: int, pad: int = 0x20):
    """{slot: gram bytes}: gram (n, i) lies at (the grams of the orders before n) + i"""
    slots, base, last_n = {}, 0, None
    for n, i, g in token_grams(token, min_n, max_n, pad):
        if n != last_n and last_n is not None:
            base = len(slots)
        last_n = n
        assert base + i not in slots
        slots[base + i] = g
    return slots


def row_grams(tokens, min_n: int, max_n: int, pad: int = 0x20):
    """the grams (bytes) of one string's tokens, in order"""
    return [g for t in tokens for _, _, g in token_grams(t, min_n, max_n, pad)]
