"""Byte streams for the decode tests (tests/test_gpu_utf8_decode.py runs them on the device, tests/test_utf8_decode_host.py runs
every one of them through the scalar reference and proves by census that they reach what they claim to reach).  Plain data: nothing
here calls the library."""
import numpy as np

TAIL = (0x00, 0x41, 0x7F, 0x80, 0x81, 0x9F, 0xA0, 0xBE, 0xBF, 0xC0, 0xE3, 0xFF)   # b2 / b3 of the windows
CHUNK, WAVE_BYTES, BLOCK = 16, 1024, 4096      # the staged decoder: bytes per thread, per wave of 64 threads, per workgroup
EDGES = (4, 16, 1024, 4096, 8192)              # dword, chunk, wave (lanes 63 | 64), block, second block
FILLER = b"ab cd.e f@g "


def windows(b0_lo=0, b0_hi=256):
    """uint8[N, 4]: every b0 in [b0_lo, b0_hi) with every b1, b2 and b3 over TAIL"""
    t = np.array(TAIL, np.uint8)
    b0, b1, b2, b3 = np.meshgrid(np.arange(b0_lo, b0_hi, dtype=np.uint8), np.arange(256, dtype=np.uint8), t, t, indexing="ij")
    return np.stack([b0.ravel(), b1.ravel(), b2.ravel(), b3.ravel()], axis=1)


def window_stream():
    """(a) every window with b0 >= 0xC0, each followed by one ASCII byte: period 5, so that every phase of dword, chunk, wave and
    block occurs; 64 * 256 * 144 * 5 bytes"""
    w = windows(0xC0)
    out = np.empty((w.shape[0], 5), np.uint8)
    out[:, :4] = w
    out[:, 4] = ord("a")
    return out.ravel()


def cut_every(total, step):
    """byte offsets of strings of `step` bytes (the last one shorter)"""
    return np.append(np.arange(0, total, step, dtype=np.int64), np.int64(total))


def filler(n):
    return (FILLER * (n // len(FILLER) + 1))[:n]


# ---- (b) every sequence at every edge --------------------------------------------------------------------------------------
CHARS = (b"Z", b"\xc3\xa9", b"\xe6\x97\xa5", b"\xf0\x9f\xa4\x93")


def sequences():
    seqs = list(CHARS)
    seqs += [c[:len(c) - cut] for c in CHARS for cut in (1, 2, 3) if cut < len(c)]      # each cut by 1..3 bytes
    seqs += [b"\xff", b"\xc3\xe6\xf0\xff\xc3"]                                          # a lone 0xFF; five lone leads in a row
    seqs += [c + b"\x80\xbf\x80\xbf\x80"[:n] for c in CHARS for n in range(1, 6)]        # 1..5 stray continuation bytes
    return seqs


SEGMENT = 3 * BLOCK      # one placement of a sequence at all five edges; a multiple of the block, so that phases survive joining


def edge_segment(seq, d):
    """SEGMENT bytes of filler with `seq` at E + d for every edge E (a sequence has at most 9 bytes, the nearest two edges are 12
    apart: the placements do not touch)"""
    buf = bytearray(filler(SEGMENT))
    for E in EDGES:
        buf[E + d:E + d + len(seq)] = seq
    return bytes(buf)


def edge_stream():
    """every sequence at every edge and every d in -4..0, filler behind it: one batch, one string per segment"""
    segs = [edge_segment(s, d) for s in sequences() for d in range(-4, 1)]
    return np.frombuffer(b"".join(segs), np.uint8), np.arange(len(segs) + 1, dtype=np.int64) * SEGMENT


def end_of_batch_cases():
    """batches that end 0, 1, 2 or 3 bytes behind a lead byte at E + d: (bytes, position of the lead).  The bytes behind the lead
    are the first bytes of a sequence (or filler where it is shorter)."""
    tails = sorted({(s + FILLER)[:1 + t] for s in sequences() for t in range(4)})
    return [(filler(E + d) + tail, E + d) for tail in tails for E in EDGES for d in range(-4, 1)]


def census(streams):
    """what a list of byte strings reaches: {(sequence length, dword phase)}, {(edge kind, bytes in front of the edge)} for
    sequences that span an edge, and the classes of `have` (bytes that exist behind a chunk: 0 for <= 0, 1, 2, 3 for >= 3) seen by
    leads whose window leaves their chunk"""
    phases, spans, haves = set(), set(), set()
    for data in streams:
        n = len(data)
        for i, b0 in enumerate(data):
            if b0 < 0xC0:
                if b0 < 0x80:
                    phases.add((1, i & 3))
                continue
            length = 2 + (b0 >= 0xE0) + (b0 >= 0xF0)
            phases.add((length, i & 3))
            whole = i + length <= n and all((b & 0xC0) == 0x80 for b in data[i + 1:i + length])
            for kind in (4, CHUNK, WAVE_BYTES, BLOCK):
                edge = (i // kind + 1) * kind                 # the first edge of this kind behind the lead
                if whole and edge < i + length:
                    spans.add((kind, edge - i))
            chunk_end = (i // CHUNK + 1) * CHUNK
            if i + length > chunk_end:
                haves.add(max(0, min(3, n - chunk_end)))
    return phases, spans, haves


# ---- (c) string starts -----------------------------------------------------------------------------------------------------
def string_start_case():
    """(u8, byte_off): a string start at every offset 0..15 of a chunk, on the lead and on each continuation byte of 1-, 2-, 3- and
    4-byte chars; runs of 70 empty strings; empty strings at the end of the batch; starts on both sides of the wave and block edges"""
    slots = [(c, j, o) for c in CHARS for j in range(len(c)) for o in range(16)]
    buf = bytearray(filler(64 * len(slots) + 64))
    starts = [0]
    for idx, (c, j, o) in enumerate(slots):
        p = 64 * idx + 16 + o                    # the start: byte j of the char
        buf[p - j:p - j + len(c)] = c
        starts.append(p)
    assert len(buf) > 2 * BLOCK
    for E in (WAVE_BYTES, BLOCK):               # a 4-byte char across the edge, strings starting on each of its bytes and around it
        buf[E - 2:E + 2] = CHARS[3]
        starts += [E - 3, E - 2, E - 1, E, E + 1, E + 2]
    starts += [64 * 5 + 16 + 5] * 70 + [BLOCK - 1] * 70 + [64 * 40 + 16 + 9] * 70      # runs of empty strings
    total = len(buf)
    starts = sorted(starts) + [total] * 71       # empty strings at byte_off == total, then the closing offset
    return np.frombuffer(bytes(buf), np.uint8), np.array(starts, np.int64)


def tiny_batches():
    """(u8, byte_off) for total_bytes = 1, 15, 16, 17, each once ending with a complete char and once with a sequence cut short"""
    out = []
    for total in (1, 15, 16, 17):
        for tail in (b"\xe6\x97\xa5", b"\xf0\x9f\xa4", b"\xc3", b"z"):
            data = (filler(32) + tail)[-total:]
            out.append((np.frombuffer(data, np.uint8), np.array([0, total], np.int64)))
            if total > 2:
                out.append((np.frombuffer(data, np.uint8), np.array([0, 0, 1, total - 1, total, total], np.int64)))
    return out


# ---- (d) all scalar values -------------------------------------------------------------------------------------------------
def all_scalars_stream(prefix=0):
    """all 0x110000 code points in ascending order, surrogates as 3-byte forms, no separators, behind `prefix` ASCII bytes"""
    text = np.arange(0x110000, dtype="<u4").tobytes().decode("utf-32-le", "surrogatepass")
    return np.frombuffer(b"abc"[:prefix] + text.encode("utf-8", "surrogatepass"), np.uint8)


def big_stream(min_bytes):
    """(e) more than min_bytes: the window stream, then the scalar values (prefix 1, 2, ...) as often as it takes (for 4096 blocks
    of 4096 bytes: twice -- the window stream and one copy are 16 185 216 bytes, short of 16 MiB)"""
    parts, k = [window_stream()], 1
    size = parts[0].size
    while size <= min_bytes:
        parts.append(all_scalars_stream(k % 4))
        size += parts[-1].size
        k += 1
    return np.concatenate(parts)


# ---- (g) lone lead bytes, no continuation byte -----------------------------------------------------------------------------
LONE_CHUNKS = (b"a\xc3 b\xff, \xe6 x\xf0", b"see me@x.org \xe3", b"\xf4#tag ", b"http://a.b/\xc3?", b" ", b"X1 \xd0\xd0 y", b".@you\xff\xff")


def lone_leads_blob(n_bytes, seed):
    rng = np.random.default_rng(seed)
    parts, size = [LONE_CHUNKS[0]], len(LONE_CHUNKS[0])
    while size < n_bytes:
        parts.append(LONE_CHUNKS[int(rng.integers(0, len(LONE_CHUNKS)))])
        size += len(parts[-1])
    return b"".join(parts)
