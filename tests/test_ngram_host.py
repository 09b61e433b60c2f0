"""Word n-grams of the term counts (include/latok_hip.h: latok_ngram_counts_utf8_bytes_batch,
latok_hashed_ngram_counts_utf8_bytes_batch), the parts that need no device: ngram_text.h, compiled by g++ (once more with the address
and undefined-behaviour sanitizers, as a stand-alone program), hashes grams whose tokens lie apart in a poisoned buffer that ends
with the aligned dword of the last byte, and gives MurmurHash3 of sep.join(tokens) by tests/helpers/murmur3_ref.py -- every carry
count against every shift, a finish behind every token, long tokens and a long gram --; its compare tells a gram from words that
differ in one byte, in where the separator stands, or in length; the entry points exist in the library, the header and
latok_amd/_lib.py with one arity; bad n-gram arguments are refused before any device is asked for, with nothing written."""
import ctypes as C
import itertools
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers.murmur3_ref import SEEDS, murmur3_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"latok_ngram_counts_utf8_bytes_batch": 17, "latok_hashed_ngram_counts_utf8_bytes_batch": 18}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    """the stand-alone program, built by plain g++ and once more with -fsanitize=address,undefined; it is run directly"""
    exe = tmp_path_factory.mktemp("ngram_" + request.param) / "ngram_harness"
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "ngram_harness.cpp"), "-o", str(exe)])

    def run(script, poison=0xA5):
        out = subprocess.run([str(exe)], input="%02x\n" % poison + script, capture_output=True, text=True)
        assert out.returncode == 0, ({2: "a text load left the buffer", 3: "a blob load left the blob"}.get(out.returncode, out.returncode),
                                     out.stderr[-2000:])
        return out.stdout.splitlines()

    return run


def _text(tokens, align, gap):
    return " ".join("%d %s" % (align if k == 0 else gap, t.hex()) for k, t in enumerate(tokens))


def _hash_line(tokens, seed, sep, align, gap):
    return "H %x %x %d %s" % (seed, sep, len(tokens), _text(tokens, align, gap))


def _want(tokens, seed, sep):
    """the finish behind every token: the hash of every order that starts at tokens[0]"""
    return ["%08x" % murmur3_ref(bytes([sep]).join(tokens[:k + 1]), seed) for k in range(len(tokens))]


def _check(harness, cases, poisons=(0x00, 0xFF, 0xA5)):
    """cases: (tokens, seed, sep, align, gap)"""
    script = "\n".join(_hash_line(*c) for c in cases) + "\n"
    want = [_want(c[0], c[1], c[2]) for c in cases]
    for poison in poisons:       # what surrounds a token in its dwords must not reach the hash
        got = [line.split() for line in harness(script, poison)]
        assert len(got) == len(cases)
        bad = [(c[3], c[4], [len(t) for t in c[0]], g, w) for c, g, w in zip(cases, got, want) if g != w]
        assert not bad, (poison, len(bad), bad[:5])


def _grid_cases():
    rng = random.Random(15)
    cases = []
    for n in (1, 2, 3):
        for lens in itertools.product(range(1, 10), repeat=n):
            tokens = [bytes(rng.randrange(1, 256) for _ in range(m)) for m in lens]
            for align in range(4):
                for gap in (0, 1, 5):
                    if n == 1 and gap:
                        continue
                    cases.append((tokens, SEEDS[(align + gap) % len(SEEDS)], 0x20, align, gap))
    return cases


GRID = _grid_cases()


def test_every_carry_count_against_every_shift(harness):
    """token lengths 1..9 for 1, 2 and 3 tokens, start alignments 0..3, gaps of 0, 1 and 5 bytes between the tokens"""
    assert len(GRID) == 9 * 4 + (81 + 729) * 12
    _check(harness, GRID)


@pytest.mark.parametrize("sep", [0x00, 0x20, 0xFF])
def test_separators_and_seeds(harness, sep):
    rng = random.Random(sep)
    cases = []
    for seed in SEEDS:
        for _ in range(40):
            tokens = [bytes(rng.randrange(256) for _ in range(rng.randrange(1, 14))) for _ in range(rng.randrange(1, 9))]
            cases.append((tokens, seed, sep, rng.randrange(4), rng.choice((0, 1, 2, 3, 5, 17))))
    _check(harness, cases)


def test_long_tokens_and_a_finish_behind_every_token_of_one_stream(harness):
    rng = random.Random(257)
    tok = lambda m: bytes(rng.randrange(256) for _ in range(m))
    cases = []
    for align in range(4):
        for big in (257, 258, 259, 260, 1000):
            cases.append(([tok(3), tok(big), tok(2)], 7, 0x20, align, 1))
            cases.append(([tok(big), tok(1), tok(big + 1)], 0xFFFFFFFF, 0x2D, align, 0))
        cases.append(([tok(1 + (k * 5) % 11) for k in range(8)], 0x9747B28C, 0x20, align, 3))   # kNgMax finishes of one stream
    cases.append(([tok(40000), tok(2), tok(25535)], 1, 0x20, 1, 2))                             # grams of 2^16 + 3 bytes
    cases.append(([tok((1 << 16) - 10), tok(12)], 0, 0x20, 3, 5))
    assert all(len(b" ".join(c[0])) == (1 << 16) + 3 for c in cases[-2:])
    _check(harness, cases, poisons=(0xA5,))


def _equal(harness, tokens, word, sep=0x20, align=0, gap=1, poison=0xA5):
    out = harness("E %x %d %s %s\n" % (sep, len(tokens), _text(tokens, align, gap), word.hex()), poison)
    assert out in (["0"], ["1"]), out
    return out == ["1"]


def test_the_compare_tells_a_gram_from_its_neighbours(harness):
    rng = random.Random(3)
    for lens in [(1,), (4,), (5,), (2, 1), (1, 2), (3, 4), (4, 4), (4, 3), (7, 9), (1, 1, 1), (3, 5, 2), (8, 8, 8), (2, 300, 5), (1,) * 8]:
        tokens = [bytes(rng.randrange(0x21, 0x7F) for _ in range(m)) for m in lens]
        word = b" ".join(tokens)
        for align in range(4):
            for gap in (0, 1, 5):
                for poison in (0x00, 0xFF):
                    assert _equal(harness, tokens, word, align=align, gap=gap, poison=poison), (lens, align, gap)
        flips = [0, len(word) - 1] + [i for i, b in enumerate(word) if b == 0x20]                # first, last, every separator
        for i in flips:
            other = word[:i] + bytes([word[i] ^ 0x01]) + word[i + 1:]
            assert not _equal(harness, tokens, other, align=i % 4), (lens, i)
        for other in (word[:-1], word + b"\x00", word + b"x", b"", word[1:]):                   # the wrong length
            if other:
                assert not _equal(harness, tokens, other), (lens, other[:16])
    assert _equal(harness, [b"ab", b"c"], b"ab c") and not _equal(harness, [b"ab", b"c"], b"a bc")   # the separator one position off
    assert _equal(harness, [b"a", b"bc"], b"a bc") and not _equal(harness, [b"a", b"bc"], b"ab c")
    assert _equal(harness, [b"new", b"york"], b"new york") and not _equal(harness, [b"new", b"york"], b"new_york")
    assert _equal(harness, [b"new", b"york"], b"new_york", sep=0x5F) and _equal(harness, [b"a", b"b"], b"a\x00b", sep=0x00)
    assert _equal(harness, [b"a", b"b"], b"a\xffb", sep=0xFF) and not _equal(harness, [b"a", b"b"], b"a\xffb", sep=0x00)


# ---- the surface -----------------------------------------------------------------------------------------------------------
def _header_decl(name):
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    m = re.search(r"^int %s\((.*?)\);" % name, text, re.S | re.M)
    assert m, "%s is not declared in include/latok_hip.h" % name
    args = re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " "))
    return [a.strip() for a in args.split(",")]


def ngram_limits():
    from latok_amd import _lib
    fn = _lib.load().latok_debug_ngram_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(2, np.int64)
    assert fn(out.ctypes.data, 2) == 2
    return int(out[0]), int(out[1])


def test_entry_points_are_exported_declared_and_bound(tmp_path):
    from latok_amd import _lib, batch
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "latok_amd", "liblatok_hip.so")], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name, n_args in ENTRIES.items():
        assert name in exported, name
        args = _header_decl(name)
        res, bound = _lib.SIGNATURES[name]
        assert res is C.c_int and len(bound) == len(args) == n_args, (name, len(bound), len(args))
        assert getattr(lib, name).argtypes == bound
    block, ng_max = ngram_limits()
    assert ng_max == 8 and block >= 64 and block % 64 == 0
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    comment = text[:text.index("int latok_ngram_counts_utf8_bytes_batch")].rsplit("/*", 1)[1]
    for needle in ("g(n, i)", "sep", "min_n", "max_n", "oov[s]", "MurmurHash3", "THREE times", "2^31", "LATOK_ERR_INVALID"):
        assert needle in comment, needle
    strict = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c"]
    subprocess.check_call(strict + [os.path.join(ROOT, "examples", "ngram_counts_utf8.c"), "-o", str(tmp_path / "example.o")])
    import inspect
    for name in ("term_counts_utf8_csr", "term_counts_utf8_batch", "term_counts_batch", "hashed_term_counts_utf8_csr",
                 "hashed_term_counts_utf8_batch", "hashed_term_counts_batch"):
        p = inspect.signature(getattr(batch, name)).parameters
        assert p["ngram_range"].default == (1, 1) and p["sep"].default == b" ", name


def test_bad_ngram_arguments_are_refused_before_any_device_with_nothing_written():
    code = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import _lib, batch
lib = _lib.load()
u8, boff = np.frombuffer(b"abc def", np.uint8), np.array([0, 7], np.int64)
indptr, idx, dat = np.full(2, -7, np.int64), np.full(8, 0x5A5A5A5A, np.int32), np.full(8, 0x5A5A5A5A, np.int32)
nnz, ng = C.c_int64(-3), C.c_int64(-3)
def hashed(min_n, max_n, sep, flags=0):
    return lib.latok_hashed_ngram_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, 0, 1 << 20, 1, min_n, max_n, sep, indptr.ctypes.data,
                                                          idx.ctypes.data, dat.ctypes.data, 8, C.byref(nnz), C.byref(ng), flags, None)
def vocab(min_n, max_n, sep, flags=0):
    return lib.latok_ngram_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, None, min_n, max_n, sep, indptr.ctypes.data, None,
                                                   idx.ctypes.data, dat.ctypes.data, 8, C.byref(nnz), C.byref(ng), flags, None)
for call in (hashed, vocab):
    for min_n, max_n, sep, needle in ((0, 1, 32, "min_n"), (-1, 2, 32, "min_n"), (2, 1, 32, "max_n"), (1, 9, 32, "max_n"), (9, 9, 32, "max_n"),
                                      (1, 2, -1, "sep"), (1, 2, 256, "sep")):
        rc = call(min_n, max_n, sep)
        assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), (min_n, max_n, sep, rc, _lib.last_error())
    assert call(1, 2, 32, flags=4) == _lib.ERR_INVALID and "flag" in _lib.last_error()
    assert call(1, 2, 32) == _lib.ERR_NOT_INIT and call(1, 8, 0) == _lib.ERR_NOT_INIT and call(8, 8, 255) == _lib.ERR_NOT_INIT
assert (indptr == -7).all() and (idx == 0x5A5A5A5A).all() and (dat == 0x5A5A5A5A).all() and nnz.value == -3 and ng.value == -3
# the Python layer refuses the same before it asks for a device
for kw in (dict(ngram_range=(0, 1)), dict(ngram_range=(2, 1)), dict(ngram_range=(1, 9)), dict(ngram_range=(1,)), dict(ngram_range=(1.5, 2)),
           dict(ngram_range=(1, 2), sep=b"ab"), dict(ngram_range=(1, 2), sep=b""), dict(ngram_range=(1, 2), sep=300)):
    for call in (lambda: batch.hashed_term_counts_utf8_csr(u8, boff, **kw), lambda: batch.hashed_term_counts_utf8_batch([b"abc def"], **kw),
                 lambda: batch.hashed_term_counts_batch(["abc def"], **kw)):
        try:
            call()
        except ValueError as e:
            continue
        raise SystemExit("no ValueError for %%r" %% (kw,))
print("ok")
""" % ROOT
    env = dict(os.environ, LATOK_DEVICE="4095")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)
