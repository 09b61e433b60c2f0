"""Joined token text (include/latok_hip.h: latok_join_tokens_utf8_bytes_batch, latok_flow_join_tokens_utf8_bytes), the parts that
need no device: the two entry points exist in the library, the header and latok_amd/_lib.py with one arity; the header stays C99
and the example compiles; the body / head lane math of lane_math.h, compiled on the host, agrees with a per-byte definition; the
Python wrappers refuse a bad separator before they touch the library; nothing is computed without a device; and the ranges a
flow batch notes keep a second batch ordered behind the first, also under an "unbounded" capacity."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKING, FLOW = "latok_join_tokens_utf8_bytes_batch", "latok_flow_join_tokens_utf8_bytes"
M64 = (1 << 64) - 1


def _header_decl(name):
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    m = re.search(r"^int %s\((.*?)\);" % name, text, re.S | re.M)
    assert m, "%s is not declared in include/latok_hip.h" % name
    args = re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " "))
    return [a.strip() for a in args.split(",")]


def test_entry_points_are_exported_declared_and_bound():
    from latok_amd import _lib, batch
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "latok_amd", "liblatok_hip.so")], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name, n_args in ((BLOCKING, 12), (FLOW, 11)):
        assert name in exported, name
        args = _header_decl(name)
        res, bound = _lib.SIGNATURES[name]
        assert res is C.c_int and len(bound) == len(args) == n_args, (name, len(bound), len(args))
        for a, b in zip(args, bound):
            if a.startswith("int64_t* n_out_bytes"):
                assert b is C.POINTER(C.c_int64)
                continue
            want = C.c_void_p if "*" in a else (C.c_int64 if a.startswith("int64_t") else C.c_int)
            assert b is want, (name, a, b)
        assert getattr(lib, name).argtypes == bound
    for name in ("join_tokens_utf8_csr", "join_tokens_utf8_batch", "join_tokens_batch", "flow_join_tokens_utf8_bytes"):
        assert callable(getattr(batch, name)), name
    # the header comment carries the definition and cites the reference
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    for name in (BLOCKING, FLOW):
        comment = text[:text.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert "default_tokenizer.py:149-160" in comment and "sep.join" in comment, name


def test_header_with_the_new_calls_is_c99_and_the_example_compiles(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "latok_hip.h"\n'
                   "int f(const uint8_t* u, const int64_t* o, uint8_t* out, int64_t* off, int32_t* c, int64_t* n, int64_t* r) {\n"
                   "    return latok_join_tokens_utf8_bytes_batch(u, o, 1, -1, ' ', out, 64, off, c, n, LATOK_OUT_INT32, NULL) +\n"
                   "           latok_flow_join_tokens_utf8_bytes(u, o, 1, -1, '\\n', out, 64, off, c, r, LATOK_OUT_INT32);\n}\n")
    strict = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c"]
    subprocess.check_call(strict + [str(src), "-o", str(tmp_path / "use.o")])
    subprocess.check_call(strict + [os.path.join(ROOT, "examples", "join_tokens_utf8.c"), "-o", str(tmp_path / "example.o")])


# ---- the lane math against a per-byte definition ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("join_planes") / "join_planes_harness"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "join_planes_harness.cpp"), "-o", str(exe)])

    def run(x, nn, r, f_in=0, b_in=0, q_in=0):
        text = "%d %d %d %d\n" % (len(x), f_in, b_in, q_in) + "".join("%x %x %x\n" % t for t in zip(x, nn, r))
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == 2 * len(x)
        return [int(v, 16) for v in out[0::2]], [int(v, 16) for v in out[1::2]]

    return run


def _bits(words, n):
    return [(words[i >> 6] >> (i & 63)) & 1 for i in range(n)]


def _per_byte(x, nn, r, f_in, b_in, q_in):
    """the definition, byte by byte.  A token is [boundary, next boundary); its body runs from its first to its last non-SPACE
    byte; head = the first body byte of a token that is not the first kept token of its string.  f_in / q_in: a non-SPACE byte of
    the open token / string lies in front of byte 0; b_in: one of the last token lies behind the last byte."""
    n = 64 * len(x)
    X, N, R = _bits(x, n), _bits(nn, n), _bits(r, n)
    body, head = [0] * n, [0] * n
    starts = [i for i in range(n) if X[i]]
    segs = [(0, starts[0] if starts else n)] + [(a, b) for a, b in zip(starts, starts[1:] + [n])]
    seen = q_in                                # a kept token earlier in the current string
    for a, b in segs:
        if a == b:
            continue
        # (string starts are token starts in real data; here any byte may begin a string: the string state resets where R is set)
        ns = [i for i in range(a, b) if N[i]]
        first_piece = a == 0 and not X[0]      # the token open at byte 0 continues one from in front
        lo = a if (first_piece and f_in) else (ns[0] if ns else None)
        hi = b - 1 if (b == n and b_in) else (ns[-1] if ns else None)
        if lo is None and hi is not None:
            lo = b                             # only what lies behind is non-SPACE: no body byte here
        if hi is None and lo is not None:
            hi = a - 1
        for i in range(a, b):
            if R[i]:
                seen = 0
            if lo is not None and hi is not None and lo <= i <= hi:
                body[i] = 1
            if N[i]:
                if ns and i == ns[0] and not (first_piece and f_in) and seen and not R[i]:
                    head[i] = 1
                seen = 1
    pack = lambda v: [sum(v[64 * w + k] << k for k in range(64)) for w in range(len(x))]
    return pack(body), pack(head)


def _check(harness, x, nn, r, f_in=0, b_in=0, q_in=0):
    got = harness(x, nn, r, f_in, b_in, q_in)
    want = _per_byte(x, nn, r, f_in, b_in, q_in)
    assert got[0] == want[0], ("body", f_in, b_in, q_in)
    assert got[1] == want[1], ("head", f_in, b_in, q_in)


def _rand_word(rng, density):
    return sum(1 << k for k in range(64) if rng.random() < density)


def test_lane_math_random_word_sequences_with_every_carry_in(harness):
    rng = random.Random(20240)
    for trial in range(120):
        n = rng.choice([1, 2, 3, 5, 64, 65, 130])
        dx, dn, dr = rng.choice([0.0, 0.02, 0.2, 0.6]), rng.choice([0.0, 0.03, 0.5, 0.97, 1.0]), rng.choice([0.0, 0.01, 0.1])
        x = [_rand_word(rng, dx) for _ in range(n)]
        nn = [_rand_word(rng, dn) for _ in range(n)]
        r = [_rand_word(rng, dr) for _ in range(n)]
        x = [a | b for a, b in zip(x, r)]          # a string start is a token start (splits[0] = 1)
        for carries in range(8):
            _check(harness, x, nn, r, carries & 1, (carries >> 1) & 1, (carries >> 2) & 1)


@pytest.mark.parametrize("n_words", [1, 2, 65, 70, 200])
def test_lane_math_one_token_over_many_words(harness, n_words):
    """one token over 1, 2 and >= 65 words: all non-SPACE; all SPACE (no body at all); its only non-SPACE byte its first, its last,
    one in the middle; a long whitespace prefix of a string in front of its first kept token"""
    zeros = [0] * n_words
    last = n_words - 1
    for carries in range(8):
        f, b, q = carries & 1, (carries >> 1) & 1, (carries >> 2) & 1
        _check(harness, [1] + zeros[1:], [M64] * n_words, [1] + zeros[1:], f, b, q)
        _check(harness, [1] + zeros[1:], zeros, [1] + zeros[1:], f, b, q)                      # an all-SPACE token
        _check(harness, zeros, zeros, zeros, f, b, q)                                          # ... in the middle of a longer one
        _check(harness, [1] + zeros[1:], [1] + zeros[1:], zeros, f, b, q)
        _check(harness, [1] + zeros[1:], zeros[:last] + [1 << 63], [1] + zeros[1:], f, b, q)   # only non-SPACE byte: its last
        mid = list(zeros)
        mid[n_words // 2] = 1 << 17
        _check(harness, [1] + zeros[1:], mid, zeros, f, b, q)
    # a string that opens with whitespace tokens (each its own token) before two kept tokens: the first has no separator
    x = [M64] * n_words
    nn = zeros[:last] + [(1 << 40) | (1 << 50)]
    _check(harness, x, nn, [1] + zeros[1:])
    got_body, got_head = harness(x, nn, [1] + zeros[1:])
    assert got_head[last] == 1 << 50 and got_body[last] == (1 << 40) | (1 << 50)


def test_lane_math_a_string_start_in_every_bit_position(harness):
    """two strings 'ab cd' + 'ef gh' (each char its own run, a boundary at every word start) with the second string starting at
    every bit of the middle word: its first kept token never gets a separator, its second always does"""
    for p in range(64):
        n = 3 * 64
        X, N, R = [0] * n, [0] * n, [0] * n
        s1 = 64 + p
        R[0] = R[s1] = 1
        for start in (0, s1):
            for k, (tok, nsp) in enumerate([(1, 1), (1, 0), (1, 1), (1, 0), (1, 1)]):
                if start + 3 * k < n:
                    X[start + 3 * k] = tok
                    N[start + 3 * k] = nsp
                    if nsp and start + 3 * k + 1 < n:
                        N[start + 3 * k + 1] = 1
        pack = lambda v: [sum(v[64 * w + k] << k for k in range(64)) for w in range(3)]
        x, nn, r = pack(X), pack(N), pack(R)
        _check(harness, x, nn, r)
        body, head = harness(x, nn, r)
        H = _bits(head, n)
        assert H[s1] == 0 and H[s1 + 6] == 1 and H[0] == 0 and H[6] == 1, p


def _rows_from_planes(u8, boff, body, head, sep):
    """the ranks of the join kernel, byte by byte: body byte i goes to (body bits before i) + (head bits at or before i), its
    separator one in front; out_off[s] = items before byte_off[s]"""
    n = len(u8)
    B, H = _bits(body, n), _bits(head, n)
    out = bytearray()
    rank_at = []
    for i in range(n):
        rank_at.append(len(out))
        if H[i]:
            out.append(sep)
        if B[i]:
            out.append(u8[i])
    rank_at.append(len(out))
    off = [rank_at[b] for b in boff]
    return [bytes(out[a:b]) for a, b in zip(off[:-1], off[1:])]


def test_planes_of_oracle_masks_give_the_reference_rows(harness, oracle):
    """the masks the byte-space tile kernel leaves, rebuilt from the oracle (boundary bits at lead bytes, the SPACE plane smeared over
    a char's continuation bytes), through the lane math and the rank rule: the rows are sep.join(tokenize(text)) of the reference"""
    from conftest import ALPHABETS, random_strings
    rng = random.Random(11)
    texts = ["This is a #test! Testing, Testing, 1 2 3", "a,b", "", "   ", "x", "　全角　空白　", " lead and trail \t", "see http://a.b/c or me@x.org"]
    texts += random_strings(rng, 300, 0, 70, ALPHABETS["mixed"]) + ["w" * 200 + " " * 150 + "z", " " * 300 + "late, token"]
    texts = [t for t in texts if "\ud800" not in t]
    X, N, R, u8, boff = [], [], [], bytearray(), [0]
    for t in texts:
        vals = oracle.split_values(t) if t else []
        for k, ch in enumerate(t):
            b = ch.encode("utf-8")
            X += [1 if vals[k] else 0] + [0] * (len(b) - 1)
            N += [0 if ch.isspace() else 1] * len(b)
            R += [1 if k == 0 else 0] + [0] * (len(b) - 1)
            u8 += b
        boff.append(len(u8))
    n_words = (len(u8) + 63) // 64
    pad = [0] * (64 * n_words - len(u8))
    pack = lambda v: [sum((v + pad)[64 * w + k] << k for k in range(64)) for w in range(n_words)]
    body, head = harness(pack(X), pack(N), pack(R))
    for sep in (b" ", b"\x00"):
        rows = _rows_from_planes(bytes(u8), boff, body, head, sep[0])
        want = [sep.join(tok.encode("utf-8") for tok in oracle.tokenize(t)) if t.strip() else b"" for t in texts]
        assert rows == want, next((t, r, w) for t, r, w in zip(texts, rows, want) if r != w)
    assert len(b"".join(rows)) <= 2 * len(u8)


# ---- Python argument checks ------------------------------------------------------------------------------------------------
def test_a_bad_separator_is_a_value_error_before_any_device():
    """LATOK_DEVICE names a device no machine has: anything that reached the library's init would raise RuntimeError instead"""
    code = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import batch
u8, boff = np.frombuffer(b"abc def", np.uint8), np.array([0, 7], np.int64)
bad_bytes = (b"", b"ab", " ", "ab", None, -1, 256, 1.5, True)
for sep in bad_bytes:
    for call in (lambda: batch.join_tokens_utf8_csr(u8, boff, sep), lambda: batch.join_tokens_utf8_batch([b"abc def"], sep)):
        try:
            call()
        except ValueError:
            continue
        raise SystemExit("no ValueError for sep=%%r" %% (sep,))
for sep in ("", "ab", "é", "　", b" ", None, 32):
    try:
        batch.join_tokens_batch(["abc def"], sep)
    except ValueError:
        continue
    raise SystemExit("no ValueError for str sep=%%r" %% (sep,))
for sep in (b"", b"ab", 256, "xy"):
    try:
        batch.flow_join_tokens_utf8_bytes(0x1000, 0x2000, 1, 7, 0x3000, 14, 0x4000, None, 0x5000, sep=sep)
    except ValueError:
        continue
    raise SystemExit("no ValueError in the flow wrapper for sep=%%r" %% (sep,))
try:
    batch.join_tokens_utf8_csr(u8, boff, b" ", dtype=np.int16)
    raise SystemExit("no ValueError for dtype")
except ValueError:
    pass
# a good separator gets as far as the device, and there is none: RuntimeError, no CPU fallback
for call in (lambda: batch.join_tokens_utf8_csr(u8, boff), lambda: batch.join_tokens_utf8_batch([b"abc def"], b"\n"),
             lambda: batch.join_tokens_batch(["abc def"]), lambda: batch.join_tokens_utf8_csr(u8, boff, 0),
             lambda: batch.flow_join_tokens_utf8_bytes(0x1000, 0x2000, 1, 7, 0x3000, 14, 0x4000, None, 0x5000)):
    try:
        call()
    except RuntimeError:
        continue
    raise SystemExit("no RuntimeError")
assert batch.join_tokens_utf8_batch([]) == [] and batch.join_tokens_batch([]) == []
print("ok")
""" % ROOT
    env = dict(os.environ, LATOK_DEVICE="4095")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_c_entries_refuse_bad_arguments_and_compute_nothing_without_a_device():
    code = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import _lib
lib = _lib.load()
u8, boff = np.frombuffer(b"abc def", np.uint8), np.array([0, 7], np.int64)
out, off, n, res = np.full(14, 0x5A, np.uint8), np.zeros(2, np.int64), C.c_int64(0), np.zeros(2, np.int64)
for sep in (-1, 256, 1 << 20):   # refused before anything else, initialised or not
    rc = lib.latok_join_tokens_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, sep, out.ctypes.data, 14, off.ctypes.data, None, C.byref(n), 0, None)
    assert rc == _lib.ERR_INVALID and "sep" in _lib.last_error(), rc
    rc = lib.latok_flow_join_tokens_utf8_bytes(u8.ctypes.data, boff.ctypes.data, 1, 7, sep, out.ctypes.data, 14, off.ctypes.data, None, res.ctypes.data, 0)
    assert rc == _lib.ERR_INVALID and "sep" in _lib.last_error(), rc
rc = lib.latok_join_tokens_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, 32, out.ctypes.data, 14, off.ctypes.data, None, C.byref(n), 0, None)
assert rc == _lib.ERR_NOT_INIT, rc
rc = lib.latok_flow_join_tokens_utf8_bytes(u8.ctypes.data, boff.ctypes.data, 1, 7, 32, out.ctypes.data, 14, off.ctypes.data, None, res.ctypes.data, 0)
assert rc == _lib.ERR_NOT_INIT, rc
assert (out == 0x5A).all() and not off.any()
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


# ---- the flow's routing ----------------------------------------------------------------------------------------------------
def _ranges(utf8, byte_off, out, out_off, counts, result, n_str, total_bytes, cap, flags=0):
    from latok_amd import _lib
    fn = _lib.load().latok_debug_flow_join_ranges
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    addr = np.array([utf8, byte_off, out, out_off, counts, result], np.uint64)
    lo, nb, wr = np.zeros(16, np.uint64), np.zeros(16, np.uint64), np.zeros(16, np.int32)
    n = fn(addr.ctypes.data, n_str, total_bytes, cap, flags, lo.ctypes.data, nb.ctypes.data, wr.ctypes.data, 16)
    assert n > 0
    return [(int(lo[i]), int(nb[i]), "w" if wr[i] else "r") for i in range(n)]


def _router():
    from latok_amd import _lib
    fn = _lib.load().latok_debug_flow_route
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]

    def submit(ranges):
        lo = np.array([r[0] for r in ranges], np.uint64)
        nb = np.array([r[1] for r in ranges], np.uint64)
        wr = np.array([r[2] == "w" for r in ranges], np.int32)
        d = C.c_int(0)
        s = fn(2, lo.ctypes.data, nb.ctypes.data, wr.ctypes.data, len(ranges), C.byref(d))
        assert s >= 0
        return s, d.value

    def reset():
        fn(2, None, None, None, -1, None)

    reset()
    return submit, reset


A = dict(utf8=0x1000000, byte_off=0x2000000, out=0x3000000, out_off=0x4000000, counts=0x5000000, result=0x6000000)
B = {k: v + 0x80000000 for k, v in A.items()}
N_STR, BYTES = 1000, 300000


def test_the_ranges_a_join_batch_notes():
    for flags, rec in ((0, 8), (2, 4)):
        r = _ranges(**A, n_str=N_STR, total_bytes=BYTES, cap=5000, flags=flags)
        assert sorted(r) == sorted([(A["result"], 16, "w"), (A["out"], 5000, "w"), (A["out_off"], (N_STR + 1) * 8, "w"),
                                    (A["counts"], N_STR * rec, "w"), (A["utf8"], BYTES, "r"), (A["byte_off"], (N_STR + 1) * 8, "r")])
        # the only bound: at most 2 * total_bytes can be written, whatever the capacity says
        for cap in (2 * BYTES, 2 * BYTES + 1, 1 << 40, 1 << 62, (1 << 63) - 1):
            r = _ranges(**A, n_str=N_STR, total_bytes=BYTES, cap=cap, flags=flags)
            assert (A["out"], 2 * BYTES, "w") in r and len(r) == 6, cap
    r = _ranges(**dict(A, counts=0), n_str=N_STR, total_bytes=BYTES, cap=5000)   # no counts asked for: nothing tracked for them
    assert all(nb == 0 for lo, nb, _ in r if lo == 0)


@pytest.mark.parametrize("cap", [5000, 1 << 62])
@pytest.mark.parametrize("shared", ["result", "out", "out_tail", "out_off", "counts", "utf8_written", None])
def test_a_second_join_batch_on_the_same_buffer_is_ordered_behind_the_first(shared, cap):
    submit, reset = _router()
    n_out = min(cap, 2 * BYTES)
    first = _ranges(**A, n_str=N_STR, total_bytes=BYTES, cap=cap)
    b = dict(B)
    if shared == "result":
        b["result"] = A["result"] + 8
    elif shared == "out":
        b["out"] = A["out"]
    elif shared == "out_tail":
        b["out"] = A["out"] + n_out - 1           # the last byte the first batch can write
    elif shared == "out_off":
        b["out_off"] = A["out_off"] + N_STR * 8
    elif shared == "counts":
        b["counts"] = A["counts"]
    elif shared == "utf8_written":
        b["out"] = A["utf8"] + 64
    second = _ranges(**b, n_str=N_STR, total_bytes=BYTES, cap=cap)
    assert submit(first) == (0, 0)
    assert submit(second) == ((1, 0) if shared is None else (0, 0))
    reset()
