"""Character n-grams inside tokens (include/latok_hip.h: latok_chargram_counts_utf8_bytes_batch,
latok_hashed_chargram_counts_utf8_bytes_batch), the parts that need no device: chargram_text.h, compiled by g++ (once more with the
address and undefined-behaviour sanitizers, as a stand-alone program), counts the characters of a token that lies in a poisoned buffer
ending with the aligned dword of its last byte, and gives the gram count, every gram's slot and MurmurHash3 of every gram's bytes as
tests/helpers/chargram_ref.py (list slicing over characters) and murmur3_ref.py give them -- every start alignment, characters of 1 to
4 bytes in every order, 1 to 10 characters against eight ranges, three pads, malformed bytes --; its compare tells a gram from words
that differ in one byte, in whether the pad is there, or in length; the entry points exist in the library, the header and
latok_amd/_lib.py with one arity; bad arguments are refused before any device is asked for, with nothing written."""
import ctypes as C
import inspect
import itertools
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers.chargram_ref import MALFORMED, RANGES, chars_of, gram_count, token_grams, token_slots
from helpers.murmur3_ref import SEEDS, murmur3_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"latok_chargram_counts_utf8_bytes_batch": 17, "latok_hashed_chargram_counts_utf8_bytes_batch": 18}
CHARS = {1: [b"a", b"Z", b"~"], 2: ["é".encode(), "ω".encode()], 3: ["日".encode(), "€".encode()], 4: ["🤓".encode(), "𝄞".encode()]}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    """the stand-alone program, built by plain g++ and once more with -fsanitize=address,undefined; it is run directly"""
    exe = tmp_path_factory.mktemp("chargram_" + request.param) / "chargram_harness"
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "chargram_harness.cpp"), "-o", str(exe)])

    def run(script, poison=0xA5):
        out = subprocess.run([str(exe)], input="%02x\n" % poison + script, capture_output=True, text=True)
        assert out.returncode == 0, ({2: "a text load left the token's dwords", 3: "a blob load left the blob"}.get(out.returncode, out.returncode),
                                     out.stderr[-2000:])
        return out.stdout.splitlines()

    return run


def _want(token, seed, pad, min_n, max_n):
    """what the W command prints, from the reference alone; the emitted grams as a sorted list (the walk's own order is free)"""
    slots = token_slots(token, min_n, max_n, pad)
    assert sorted(slots) == list(range(gram_count(len(chars_of(token)), min_n, max_n))) == list(range(len(token_grams(token, min_n, max_n, pad))))
    return len(chars_of(token)), len(slots), sorted((s, "%08x" % murmur3_ref(g, seed), len(g)) for s, g in slots.items())


def _check(harness, cases, poisons=(0x00, 0xFF, 0xA5)):
    """cases: (token, seed, pad, min_n, max_n, gap).  The count of characters, G(W), and per gram slot, hash and length; the byte range
    and the pad flags the walk reports must spell the same gram."""
    script = "".join("W %x %x %d %d %d %s\n" % (seed, pad, lo, hi, gap, tok.hex()) for tok, seed, pad, lo, hi, gap in cases)
    want = [_want(tok, seed, pad, lo, hi) for tok, seed, pad, lo, hi, gap in cases]
    for poison in poisons:       # what surrounds the token in its dwords must reach neither a count nor a hash
        lines = harness(script, poison)
        assert len(lines) == len(cases)
        for case, line, (n_chars, n_grams, grams) in zip(cases, lines, want):
            tok, seed, pad = case[:3]
            f = line.split()
            assert (int(f[0]), int(f[1]), int(f[2])) == (n_chars, n_grams, n_grams), (poison, case, f[:3])
            got, spelled = [], {}
            for item in f[3:]:
                slot, h, ln, gs, ge, front, back = item.split(":")
                got.append((int(slot), h, int(ln)))
                spelled[int(slot)] = bytes([pad]) * int(front) + tok[int(gs):int(ge)] + bytes([pad]) * int(back)
            assert sorted(got) == grams, (poison, case, sorted(got)[:4], grams[:4])
            assert spelled == token_slots(tok, case[3], case[4], pad), (poison, case)


def _mixed_tokens():
    """characters of 1, 2, 3 and 4 bytes in every order, and 1 .. 10 characters of mixed widths"""
    rng = random.Random(17)
    toks = [b"".join(CHARS[w][0] for w in perm) for k in (1, 2, 3, 4) for perm in itertools.permutations((1, 2, 3, 4), k)]
    for n_chars in range(1, 11):
        for _ in range(3):
            toks.append(b"".join(rng.choice(CHARS[rng.randrange(1, 5)]) for _ in range(n_chars)))
        toks.append(b"x" * n_chars)
    return toks


def test_counts_slots_and_hashes_of_every_length_against_every_range(harness):
    """L = 1 .. 10 against the eight ranges (W < n, W = n and W = n + 1 all occur), every start alignment 0 .. 3 and two further in"""
    toks = _mixed_tokens()
    assert {len(chars_of(t)) for t in toks} >= set(range(1, 11))
    lengths = {len(chars_of(t)) + 2 for t in toks}
    assert min(lengths) == 3                         # (a padded word has at least 3 characters: below order 4 no word is short)
    for lo, hi in RANGES:
        assert (hi < 2 or hi + 1 in lengths) and (hi < 3 or hi in lengths) and (hi < 4 or any(w < hi for w in lengths))
    cases = [(t, SEEDS[(k + gap) % len(SEEDS)], 0x20, lo, hi, gap) for k, t in enumerate(toks) for lo, hi in RANGES for gap in (0, 1, 2, 3, 6, 9)]
    _check(harness, cases)


@pytest.mark.parametrize("pad", [0x20, 0x00, 0xFF])
def test_pads_and_seeds(harness, pad):
    rng = random.Random(pad)
    toks = _mixed_tokens()
    cases = [(rng.choice(toks), seed, pad, lo, hi, rng.randrange(8)) for seed in SEEDS for lo, hi in RANGES for _ in range(6)]
    _check(harness, cases)


def test_malformed_bytes_are_characters_by_the_same_total_rule(harness):
    """a continuation byte first, a run of them, a truncated lead as the last byte, 0xC0 and 0xF8 .. 0xFF"""
    assert len(chars_of(b"\x80abc")) == 4 and len(chars_of(b"\x80\x81\x82")) == 1 and len(chars_of(b"ab\xe2")) == 3
    assert len(chars_of(b"\xf9\xfa\xfb")) == 3 and len(chars_of(b"\xbf\xbf\xbf\xbfx\x80\x80")) == 2
    cases = [(t, 0x9747B28C, pad, lo, hi, gap) for t in MALFORMED for lo, hi in RANGES for gap in range(4) for pad in (0x20, 0x80)]
    _check(harness, cases)


def test_a_long_token(harness):
    rng = random.Random(5)
    tok = b"".join(rng.choice(CHARS[rng.randrange(1, 5)]) for _ in range(700))
    _check(harness, [(tok, 1, 0x20, lo, hi, gap) for (lo, hi), gap in zip(RANGES, (0, 1, 2, 3, 0, 1, 2, 3))], poisons=(0xA5,))


def _equal(harness, tok, gs, ge, front, back, word, pad=0x20, gap=0, poison=0xA5):
    out = harness("E %x %d %s %d %d %d %d %s\n" % (pad, gap, tok.hex(), gs, ge, front, back, word.hex() or "-"), poison)
    assert out in (["0"], ["1"]), out
    return out == ["1"]


def test_the_compare_tells_a_gram_from_its_neighbours(harness):
    tok = "the日quick🤓é".encode()
    sp = b" "
    for gs, ge, front, back in [(0, 3, 1, 0), (0, 2, 1, 0), (1, 3, 0, 0), (3, 6, 0, 0), (0, len(tok), 1, 1), (len(tok) - 2, len(tok), 0, 1),
                                (len(tok), len(tok), 0, 1), (0, 0, 1, 0), (6, 15, 0, 0), (2, 11, 0, 0)]:
        word = sp * front + tok[gs:ge] + sp * back
        for gap in (0, 1, 2, 3, 5):
            for poison in (0x00, 0xFF):
                assert _equal(harness, tok, gs, ge, front, back, word, gap=gap, poison=poison), (gs, ge, front, back, gap)
        for i in {0, len(word) - 1, len(word) // 2}:                                    # one byte differs: first, last, middle
            other = word[:i] + bytes([word[i] ^ 0x01]) + word[i + 1:]
            assert not _equal(harness, tok, gs, ge, front, back, other, gap=i % 4), (gs, ge, i)
        for other in (word[:-1], word + b"\x00", word + b" ", b" " + word, word[1:], b""):   # the wrong length, the pad too many or missing
            assert not _equal(harness, tok, gs, ge, front, back, other), (gs, ge, other)
    assert _equal(harness, b"th", 0, 2, 1, 0, b" th") and not _equal(harness, b"th", 0, 2, 0, 0, b" th")
    assert _equal(harness, b"th", 0, 2, 0, 1, b"th ") and not _equal(harness, b"th", 0, 2, 1, 0, b"th ")       # the pad on the other side
    assert _equal(harness, b"th", 0, 2, 1, 1, b"\x00th\x00", pad=0) and not _equal(harness, b"th", 0, 2, 1, 1, b" th ", pad=0)
    assert _equal(harness, b"th", 0, 2, 1, 1, b"\xffth\xff", pad=0xFF)


# ---- the surface -----------------------------------------------------------------------------------------------------------
def _header_decl(name):
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    m = re.search(r"^int %s\((.*?)\);" % name, text, re.S | re.M)
    assert m, "%s is not declared in include/latok_hip.h" % name
    args = re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " "))
    return [a.strip() for a in args.split(",")]


def chargram_limits():
    from latok_amd import _lib
    fn = _lib.load().latok_debug_chargram_limits
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
    block, ng_max = chargram_limits()
    assert ng_max == 8 and block >= 64 and block % 64 == 0
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    comment = text[:text.index("int latok_chargram_counts_utf8_bytes_batch")].rsplit("/*", 1)[1]
    for needle in ("(b & 0xC0) != 0x80", "pad", "W = L + 2", "NO HIGHER", "G(W)", "min_n", "max_n", "oov[s]", "MurmurHash3", "THREE times", "2^31",
                   "LATOK_ERR_INVALID", 'analyzer="char"'):
        assert needle in comment, needle
    strict = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c"]
    subprocess.check_call(strict + [os.path.join(ROOT, "examples", "chargram_counts_utf8.c"), "-o", str(tmp_path / "example.o")])
    for name in ("term_counts_utf8_csr", "term_counts_utf8_batch", "term_counts_batch", "hashed_term_counts_utf8_csr",
                 "hashed_term_counts_utf8_batch", "hashed_term_counts_batch"):
        p = inspect.signature(getattr(batch, name)).parameters
        assert p["analyzer"].default == "word" and p["pad"].default == b" " and p["ngram_range"].default == (1, 1), name


def test_bad_arguments_are_refused_before_any_device_with_nothing_written():
    code = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import _lib, batch
lib = _lib.load()
u8, boff = np.frombuffer(b"abc def", np.uint8), np.array([0, 7], np.int64)
indptr, idx, dat = np.full(2, -7, np.int64), np.full(64, 0x5A5A5A5A, np.int32), np.full(64, 0x5A5A5A5A, np.int32)
nnz, ng = C.c_int64(-3), C.c_int64(-3)
def hashed(min_n, max_n, pad, flags=0):
    return lib.latok_hashed_chargram_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, 0, 1 << 20, 1, min_n, max_n, pad, indptr.ctypes.data,
                                                             idx.ctypes.data, dat.ctypes.data, 64, C.byref(nnz), C.byref(ng), flags, None)
def vocab(min_n, max_n, pad, flags=0):
    return lib.latok_chargram_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, None, min_n, max_n, pad, indptr.ctypes.data, None,
                                                      idx.ctypes.data, dat.ctypes.data, 64, C.byref(nnz), C.byref(ng), flags, None)
for call in (hashed, vocab):
    for min_n, max_n, pad, needle in ((0, 1, 32, "min_n"), (-1, 2, 32, "min_n"), (2, 1, 32, "max_n"), (1, 9, 32, "max_n"), (9, 9, 32, "max_n"),
                                      (1, 2, -1, "pad"), (1, 2, 256, "pad")):
        rc = call(min_n, max_n, pad)
        assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), (min_n, max_n, pad, rc, _lib.last_error())
    assert call(3, 5, 32, flags=4) == _lib.ERR_INVALID and "flag" in _lib.last_error()
    assert call(1, 1, 32) == _lib.ERR_NOT_INIT and call(1, 8, 0) == _lib.ERR_NOT_INIT and call(8, 8, 255) == _lib.ERR_NOT_INIT
assert (indptr == -7).all() and (idx == 0x5A5A5A5A).all() and (dat == 0x5A5A5A5A).all() and nnz.value == -3 and ng.value == -3
# the Python layer refuses the same, and a bad analyzer, before it asks for a device
bad = [dict(analyzer="char_wb", ngram_range=(0, 1)), dict(analyzer="char_wb", ngram_range=(2, 1)), dict(analyzer="char_wb", ngram_range=(1, 9)),
       dict(analyzer="char_wb", ngram_range=(1,)), dict(analyzer="char_wb", ngram_range=(1.5, 2)), dict(analyzer="char_wb", pad=b"ab"),
       dict(analyzer="char_wb", pad=b""), dict(analyzer="char_wb", pad=300), dict(analyzer="char_wb", pad=" "), dict(analyzer="char"),
       dict(analyzer="chars"), dict(analyzer=None), dict(analyzer=b"word"), dict(analyzer="WORD"), dict(analyzer=len)]
for kw in bad:
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
