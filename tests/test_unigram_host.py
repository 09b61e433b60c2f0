"""Unigram (include/latok_hip.h: latok_unigram_*), the parts that need no device: the entry points exist in the library, the header and
latok_amd/_lib.py with one arity and the header stays C99; unigram.h, compiled by g++ (once more with the address and
undefined-behaviour sanitizers, as a stand-alone program), builds its tables and cuts tokens at every alignment inside a poisoned buffer
exactly as tests/helpers/unigram_ref.py -- a plain restatement of the definition over bytes, a dict and numpy.float32 -- does: the
recorded cases of tokenizers.models.Unigram (tests/golden/unigram_hf_cases.json), seeded random vocabularies with arbitrary float32
scores (some hold every character, some none), every length 1 .. 70, ties, the marker's cases, a fused unknown run that spells a word,
a damaged table, V = 0, duplicates; a counter in the harness proves the lookup bound; the reference itself is held to the golden file and
to the `tokenizers` package where that is installed; latok_unigram_create refuses bad arguments before it asks for a device."""
import ctypes as C
import json
import os
import random
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from helpers import unigram_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"latok_unigram_create": 12, "latok_unigram_destroy": 1, "latok_unigram_info": 13, "latok_unigram_ids_utf8_bytes_batch": 14,
           "latok_unigram_padded_utf8_bytes_batch": 16}
UNK = -1
MK = ref.MARKER
SEEDS = (0, 1, 0x9747B28C, 0xFFFFFFFF)


def _f32bits(x):
    return struct.unpack("<I", struct.pack("<f", float(np.float32(x))))[0]


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "unigram_hf_cases.json"), encoding="utf-8") as f:
        return json.load(f)


def _golden_want(case):
    m = len(MK) if case["marked"] else 0
    return [(i, max(s - m, 0), e - m) for i, (s, e) in zip(case["ids"], case["offsets"])]


def _header_decl(name):
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    m = re.search(r"^int %s\((.*?)\);" % name, text, re.S | re.M)
    assert m, "%s is not declared in include/latok_hip.h" % name
    args = re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " "))
    return [a.strip() for a in args.split(",")]


# ---- the surface -----------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_declared_and_bound():
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
        for a, b in zip(args, bound):
            if a.startswith("int32_t ") and "*" not in a:
                assert b is C.c_int32, (name, a)
            elif a == "uint32_t seed":
                assert b is C.c_uint32
            elif a == "float unk_score":
                assert b is C.c_float
            elif "*" in a:
                assert b is C.c_void_p or issubclass(b, C._Pointer), (name, a, b)
            else:
                assert b is (C.c_int64 if a.startswith("int64_t") else C.c_int), (name, a, b)
    assert "latok_debug_unigram_limits" in exported
    for name in ("Unigram", "unigram_ids_utf8_csr", "unigram_ids_utf8_batch", "unigram_ids_batch", "unigram_encode_utf8_batch"):
        assert callable(getattr(batch, name)), name
    assert callable(batch.Unigram.from_vocab_file)
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    comment = text[:text.index("typedef struct latok_unigram")].rsplit("/*", 1)[1]
    for needle in ("first wins", "exactly one character", "MARKED", "(b & 0xC0) != 0x80", "VIRTUAL TEXT", "best[0] = 0.0f", "ONE float32", "strictly greater",
                   "LOWER START", "max(p - m, 0)", "(a, a)", "fuse_unk = 1", "V = 0", "PIECES", "latok_token_spans_utf8_bytes_batch", "LATOK_ERR_INVALID",
                   "byte_fallback", "n-best", "protobuf", "flow form", "EOS-only", "LATOK_DETOK_CONCAT", "trie", "normalizer"):
        assert needle in comment, needle


def test_limits_hook():
    from latok_amd import _lib
    fn = _lib.load().latok_debug_unigram_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(4, np.int64)
    assert fn(out.ctypes.data, 4) == 4
    assert out[0] > 0 and out[0] % 64 == 0 and out[1] > 0 and out[2] == 64 and out[3] == 4096
    assert fn(out.ctypes.data, 2) == 2 and fn(None, 4) < 0


def test_header_with_the_new_calls_is_c99_and_the_example_compiles(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "latok_hip.h"\n'
                   "int f(const uint8_t* u, const int64_t* o, const float* sc, int64_t* ip, int64_t* sp, int32_t* ids, int32_t* len, int64_t* n) {\n"
                   "    latok_unigram* w = NULL;\n"
                   "    int64_t a, b, c, d, e; int ml, fu, mb, dev; uint32_t seed; float us; uint8_t mk[4];\n"
                   "    int rc = latok_unigram_create(u, o, 1, sc, NULL, u, 3, -10.0f, 1, 4096, 7u, &w);\n"
                   "    rc += latok_unigram_info(w, &a, &b, &c, &d, &e, mk, &ml, &us, &fu, &mb, &seed, &dev);\n"
                   "    rc += latok_unigram_ids_utf8_bytes_batch(u, o, 1, -1, w, -1, ip, ids, sp, 64, n, NULL, 0, NULL);\n"
                   "    rc += latok_unigram_padded_utf8_bytes_batch(u, o, 1, -1, w, 0, 16, 1, 101, 102, 0, ids, len, n, 0, NULL);\n"
                   "    return rc + latok_unigram_destroy(w);\n}\n")
    strict = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c"]
    subprocess.check_call(strict + [str(src), "-o", str(tmp_path / "use.o")])
    subprocess.check_call(strict + [os.path.join(ROOT, "examples", "unigram_utf8.c"), "-o", str(tmp_path / "example.o")])


# ---- the reference ---------------------------------------------------------------------------------------------------------
GREEDY_WORDS = [b"ab", b"cd", b"abc", b"bcd", b"a", b"b", b"c", b"d"]
GREEDY_SCORES = [-1.0, -1.125, -1.0, -1.0, -4.0, -4.0, -4.0, -4.0]


def test_the_reference_gives_the_worked_cases():
    d = ref.word_dict(GREEDY_WORDS)
    us = ref.default_unk_score(GREEDY_SCORES)
    assert us == np.float32(-14.0)
    # the best path is not the greedy longest match (abc + d = -5, ab + cd = -2.125)
    assert ref.cut(b"abcd", False, d, GREEDY_SCORES, us) == [(0, 0, 2), (1, 2, 4)]
    # a marked token whose marker is no word: an unknown piece with the empty range; fused with a following unknown character
    assert ref.cut(b"ab", True, d, GREEDY_SCORES, us) == [(-1, 0, 0), (0, 0, 2)]
    assert ref.cut(b"xab", True, d, GREEDY_SCORES, us) == [(-1, 0, 1), (0, 1, 3)]
    assert ref.cut(b"xab", True, d, GREEDY_SCORES, us, fuse_unk=False) == [(-1, 0, 0), (-1, 0, 1), (0, 1, 3)]
    # the marker alone and marker + prefix
    words = GREEDY_WORDS + [MK, MK + b"ab"]
    scores = GREEDY_SCORES + [-2.0, -1.5]
    d2 = ref.word_dict(words)
    assert ref.cut(b"abcd", True, d2, scores, us) == [(9, 0, 2), (1, 2, 4)]
    assert ref.cut(b"cd", True, d2, scores, us) == [(8, 0, 0), (1, 0, 2)]
    # ties: of equal scores the lower start of the last piece stays (a + aa, not aa + a)
    d3 = ref.word_dict([b"a", b"aa"])
    assert ref.cut(b"aaa", False, d3, [-1.0, -1.0], -20.0) == [(0, 0, 1), (1, 1, 3)]
    # a fused unknown run may spell a word that the search rejected
    d4 = ref.word_dict([b"xy"])
    assert ref.cut(b"xy", False, d4, [-100.0], -1.0) == [(-1, 0, 2)]
    assert ref.cut(b"xy", False, d4, [-100.0], -1.0, fuse_unk=False) == [(-1, 0, 1), (-1, 1, 2)]
    # V = 0, a long token
    assert ref.cut(b"a\xc3\xa9b", False, {}, [], -10.0) == [(-1, 0, 4)] and len(ref.cut(b"a\xc3\xa9b", True, {}, [], -10.0, fuse_unk=False)) == 4
    assert ref.cut(b"abc", True, d, GREEDY_SCORES, us, max_bytes=2, unk=-9) == [(-9, 0, 3)]


def test_the_reference_gives_the_recorded_cases_of_the_tokenizers_package():
    doc = _golden()
    assert doc["library"] == "tokenizers" and doc["version"] and len(doc["vocabularies"]) >= 8
    n = 0
    for v in doc["vocabularies"]:
        assert all(s * 8 == int(s * 8) for s in v["scores"])
        words = [w.encode() for w in v["words"]]
        d, us = ref.word_dict(words), ref.default_unk_score(v["scores"])
        for c in v["cases"]:
            assert ref.cut(c["word"].encode(), c["marked"], d, v["scores"], us, unk=v["unk_id"]) == _golden_want(c), c
            n += 1
    assert n >= 300


def test_the_reference_agrees_with_the_tokenizers_package():
    tokenizers = pytest.importorskip("tokenizers")
    from tokenizers.models import Unigram
    rng = random.Random(7)
    alphabet = "abé日"
    for trial in range(20):
        words = ["<unk>"] + sorted({"".join(rng.choice(alphabet + "▁") for _ in range(rng.randint(1, 3))) for _ in range(rng.randint(1, 14))})
        scores = [0.0] + [-rng.randint(1, 40) / 8.0 for _ in words[1:]]
        tok = tokenizers.Tokenizer(Unigram(list(zip(words, scores)), unk_id=0, byte_fallback=False))
        d, us = ref.word_dict([w.encode() for w in words]), ref.default_unk_score(scores)
        for _ in range(40):
            text = "".join(rng.choice(alphabet + "z▁") for _ in range(rng.randint(1, 10)))
            enc = tok.encode(text, add_special_tokens=False)
            at = [0]
            for ch in text:
                at.append(at[-1] + len(ch.encode()))
            want = [(i, at[s], at[e]) for i, (s, e) in zip(enc.ids, enc.offsets)]
            assert ref.cut(text.encode(), False, d, scores, us, unk=0) == want, (words, scores, text)


# ---- unigram.h on the host ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    """the stand-alone program, built by plain g++ and once more with -fsanitize=address,undefined; it is run directly"""
    exe = tmp_path_factory.mktemp("uni_" + request.param) / "unigram_harness"
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "unigram_harness.cpp"), "-o", str(exe)])

    def run(script, poison=0xA5):
        out = subprocess.run([str(exe)], input="%02x\n" % poison + script, capture_output=True, text=True)
        assert out.returncode == 0, ({2: "a text load left the token's dwords", 3: "a table load left the table",
                                      4: "the lane state and the wide state disagree", 5: "a pair was looked up twice in one pass"}.get(out.returncode, out.returncode),
                                     out.stderr[-2000:])
        return out.stdout.splitlines()

    return run


_WANT = {}     # the reference's cut of a (vocabulary, token, marked): computed once, shared by every pad, poison and build of the harness


def _run(harness, words, scores, tokens, unk_score=None, marker=MK, fuse=True, max_bytes=4096, seed=0, ids=None, unk=UNK, pads=(0, 1, 2, 3),
         damaged=False, poisons=(0x00, 0xFF, 0xA5)):
    """every (token, marked) at every pad, against the reference and the lookup bound; returns (info of the tables, slot loads per case)"""
    d = ref.word_dict(words)
    us = ref.default_unk_score(scores) if unk_score is None else np.float32(unk_score)
    vkey = (tuple(words), tuple(_f32bits(x) for x in scores), _f32bits(us), marker, fuse, max_bytes, unk, None if ids is None else tuple(ids), damaged)
    cases = [(pad, t, mk) for t, mk in tokens for pad in pads]
    lines = ["V %x %d %d %x %s %d" % (seed, max_bytes, 1 if fuse else 0, _f32bits(us), marker.hex() or "-", len(words))]
    lines += ["%s %x %s" % ("-" if ids is None else ids[i], _f32bits(scores[i]), w.hex() or "-") for i, w in enumerate(words)]
    lines += ["F"] if damaged else []
    lines += ["T %d %d %d %s" % (pad, unk, 1 if mk else 0, t.hex()) for pad, t, mk in cases]
    info = loads = None
    with np.errstate(over="ignore"):
        for poison in poisons:      # what surrounds the token in its dwords must not reach the hash or the compare
            out = harness("\n".join(lines) + "\n", poison)
            m = re.match(r"slots (\d+) (\d+) used (\d+) (\d+) max (\d+) marker (-?\d+)$", out[0])
            assert m and len(out) == 1 + len(cases), out[:3]
            info = tuple(map(int, m.groups()))
            n_marked = len({w[len(marker):] for w in d if marker and w.startswith(marker) and len(w) > len(marker)})
            if not damaged:
                assert info[2] == len(d) and info[3] == n_marked and info[5] == d.get(marker, -1) if marker else info[5] == -1
            loads = []
            for (pad, t, mk), line in zip(cases, out[1:]):
                f = line.split()
                got = [tuple(map(int, x.split(":"))) for x in f[1:-4]]
                want = _WANT.get((vkey, t, mk))
                if want is None:
                    want = _WANT[(vkey, t, mk)] = ref.cut(t, mk, {} if damaged else d, scores, us, marker, fuse, max_bytes, unk, ids)
                assert int(f[0]) == len(got) and got == want, (poison, pad, t, mk, got, want)
                lookups, bound, emit_lookups = int(f[-4]), int(f[-3]), int(f[-2])
                # every pair of positions within the longest word's reach at most once per pass; one lookup per piece that is a word
                assert lookups <= bound and emit_lookups <= len(got), (t, lookups, bound, emit_lookups)
                n_pos = len(ref.positions((marker if mk else b"") + t)) - 1
                longest = max([len(w) for w in words] + [0])
                assert len(t) > max_bytes or bound <= n_pos * min(n_pos, longest + 1), (t, bound, n_pos, longest)
                loads.append(int(f[-1]))
    return info, loads


def _both(tokens):
    return [(t, mk) for t in tokens for mk in (False, True)]


def test_the_recorded_cases_of_the_tokenizers_package(harness):
    for v in _golden()["vocabularies"]:
        words = [w.encode() for w in v["words"]]
        tokens = [(c["word"].encode(), c["marked"]) for c in v["cases"]]
        _run(harness, words, v["scores"], tokens, unk=v["unk_id"], pads=(0, 3), poisons=(0xA5,))
        out = harness("V 0 4096 1 %x %s %d\n" % (_f32bits(ref.default_unk_score(v["scores"])), MK.hex(), len(words)) +
                      "".join("- %x %s\n" % (_f32bits(s), w.hex()) for w, s in zip(words, v["scores"])) +
                      "".join("T 1 %d %d %s\n" % (v["unk_id"], c["marked"], c["word"].encode().hex()) for c in v["cases"]))
        for c, line in zip(v["cases"], out[1:]):     # the recorded cases themselves, not only the reference
            assert [tuple(map(int, x.split(":"))) for x in line.split()[1:-4]] == _golden_want(c), c


def test_the_worked_cases(harness):
    _run(harness, GREEDY_WORDS, GREEDY_SCORES, _both([b"abcd", b"ab", b"xab", b"abcdabcd", b"dcba", b"x", b"xx", b"axxb", b"abcd" * 20]), pads=range(8))
    _run(harness, GREEDY_WORDS, GREEDY_SCORES, _both([b"abcd", b"xab", b"xx", b"axxb", b"x"]), fuse=False)
    _run(harness, GREEDY_WORDS + [MK, MK + b"ab"], GREEDY_SCORES + [-2.0, -1.5], _both([b"abcd", b"cd", b"x", b"ab"]))
    _run(harness, [b"a", b"aa", b"aaa"], [-1.0, -1.0, -1.0], _both([b"a" * n for n in range(1, 12)]), unk_score=-20.0)
    _run(harness, [b"a", b"aa", b"aaa", MK + b"a", MK], [-1.0, -2.0, -3.0, -1.0, -1.0], _both([b"a" * n for n in range(1, 12)]), unk_score=-20.0)
    for fuse in (True, False):     # a fused unknown run that spells a word
        _run(harness, [b"xy", b"q"], [-100.0, -1.0], _both([b"xy", b"xyq", b"qxy", b"xyxy"]), unk_score=-1.0, fuse=fuse)
    _run(harness, GREEDY_WORDS, GREEDY_SCORES, _both([b"abcd", b"xab"]), marker=b"")            # an empty marker: no token is marked
    _run(harness, GREEDY_WORDS + [b"#ab"], GREEDY_SCORES + [-0.5], _both([b"abcd", b"xab"]), marker=b"#")


@pytest.mark.parametrize("seed", SEEDS)
def test_random_vocabularies_with_arbitrary_float32_scores(harness, seed):
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    for alphabet in ("abc", "abé", "a日é▁"):
        chars = [c.encode() for c in alphabet]
        for n_words, singles in ((3, False), (30, True), (200, True), (40, False)):
            words = (chars if singles else []) + [b"".join(rng.choice(chars) for _ in range(rng.choice((1, 2, 2, 2, 3, 3, 4, 5)))) for _ in range(n_words)]
            words += [MK + w for w in rng.sample(words, len(words) // 3)] + ([MK] if rng.random() < 0.5 else [])
            rng.shuffle(words)
            scores = (-nrng.random(len(words), np.float32) * np.float32(12) - np.float32(0.01)).astype(np.float32)
            if n_words == 40:      # sums that round hard, and sums that overflow
                scores = (scores * np.float32(1e7)).astype(np.float32) if seed & 1 else (scores * np.float32(2.5e37)).astype(np.float32)
            letters = chars + [b"z", b"\xf0\x9f\xa4\x93"]
            tokens = [b"".join(rng.choice(letters if rng.random() < 0.3 else chars) for _ in range(rng.randint(1, 14))) for _ in range(40)]
            tokens += [w for w in words if not w.startswith(MK)][:20]
            ids = [rng.randrange(-1 << 31, 1 << 31) for _ in words] if n_words == 30 else None
            _run(harness, words, scores, _both(tokens), seed=seed, ids=ids, unk=-7 if ids else UNK, fuse=bool(n_words != 200), pads=(0, 3),
                 poisons=(0xA5,))


def test_every_length_at_every_alignment_and_malformed_bytes(harness):
    rng = random.Random(5)
    chars = [b"a", b"b", b"\xc3\xa9", b"\xe6\x97\xa5"]
    words = chars[:3] + [b"".join(rng.choice(chars) for _ in range(rng.randint(2, 5))) for _ in range(60)]
    words += [MK + w for w in words[:20]]
    scores = [-rng.randint(1, 80) / 8.0 for _ in words]
    tokens = [b"".join(rng.choice(chars) for _ in range(n))[:n] for n in range(1, 71) for _ in range(2)]      # ([:n] cuts lead bytes off at the end)
    tokens += [b"ab" * 32, b"ab" * 33, b"a" * 64, b"a" * 65, b"\xa9\xa9a", b"\xa9", b"\x97\xa5ab\xe6", b"a\xe6\x97", b"\xf0\x9f", b"\x80" * 64, b"\x80" * 70]
    _run(harness, words, scores, _both(tokens), poisons=(0x00, 0xA5))


def test_max_bytes_and_long_tokens(harness):
    words, scores = GREEDY_WORDS, GREEDY_SCORES
    for mb in (1, 2, 3, 64, 65, 80, 500):
        _run(harness, words, scores, _both([(b"abcd" * 1025)[:n] for n in (mb - 1, mb, mb + 1) if n > 0]), max_bytes=mb, pads=(0, 3), poisons=(0xA5,))
    _, loads = _run(harness, words, scores, [(b"abcd" * 1024, True), (b"x" * 4096, False), (b"abcd" * 1024 + b"a", False)], pads=(1,), poisons=(0xA5,))
    assert all(l > 0 for l in loads[:2])
    # a span longer than the longest word needs no probe: the bound is positions x reach, not positions squared
    _run(harness, [b"a", b"b"], [-1.0, -2.0], _both([b"ab" * 100]), pads=(0,), poisons=(0xA5,))


def test_a_table_without_an_empty_slot_ends_every_loop(harness):
    words = [b"w%d" % i for i in range(40)]
    info, loads = _run(harness, words, [-1.0] * 40, _both([b"w1", b"w1w2", b"other", b"w" * 50]), damaged=True, unk=-5, pads=(0, 3))
    assert all(l % info[0] == 0 and 0 < l for l in loads), (info, loads)


def test_an_empty_vocabulary_empty_words_and_duplicates(harness):
    for fuse in (True, False):
        _run(harness, [], [], _both([b"a", b"ab", b"\xc3\xa9", b"a" * 300, b"a" * 5000]), fuse=fuse)
    _run(harness, [b"", b"", b""], [-1.0, -2.0, -3.0], _both([b"a", b"ab"]))
    words = [b"a", b"b", b"ab", b"a", b"ab", b"", b"b", b"ba", MK + b"a", MK + b"a", MK, MK]
    info, _ = _run(harness, words, [-1.0, -1.0, -5.0, -0.5, -0.5, -1.0, -9.0, -1.5, -1.0, -0.25, -1.0, -0.125],
                   _both([b"ab", b"ba", b"abab", b"baba", b"aab"]), ids=[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12])
    assert info[2] == 6 and info[3] == 1 and info[5] == 10


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_create_refuses_bad_arguments_before_it_asks_for_a_device():
    code = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import _lib
lib = _lib.load()
words = np.frombuffer(b"abcde", np.uint8)
h = C.c_void_p()
def create(off, n, out=h, w=words, sc=(-1.0, -2.0), mk=b"\xe2\x96\x81", ml=None, us=-12.0, fu=1, mb=4096):
    off = np.array(off, np.int64)
    sc = np.array(sc, np.float32) if sc is not None else None
    m = np.frombuffer(mk + b"\0", np.uint8)
    return lib.latok_unigram_create(w.ctypes.data if w is not None else None, off.ctypes.data, n, sc.ctypes.data if sc is not None else None, None,
                                    m.ctypes.data, len(mk) if ml is None else ml, us, fu, mb, 0, C.byref(out) if out is not None else None)
inf, nan = float("inf"), float("nan")
for kw, needle in ((dict(off=[1, 2, 5], n=2), "start at 0"), (dict(off=[0, 3, 2], n=2), "non-decreasing"), (dict(off=[0, 2, 5], n=-1), "n_words"),
                   (dict(off=[0, 2, 5], n=1 << 31), "n_words"), (dict(off=[0, 1 << 32], n=1), "2^32"), (dict(off=[0, 2, 5], n=2, mb=0), "max_bytes"),
                   (dict(off=[0, 2, 5], n=2, mb=4097), "max_bytes"), (dict(off=[0, 2, 5], n=2, mb=-1), "max_bytes"),
                   (dict(off=[0, 2, 5], n=2, fu=2), "fuse_unk"), (dict(off=[0, 2, 5], n=2, fu=-1), "fuse_unk"),
                   (dict(off=[0, 2, 5], n=2, sc=(-1.0, inf)), "scores[1]"), (dict(off=[0, 2, 5], n=2, sc=(nan, -1.0)), "scores[0]"),
                   (dict(off=[0, 2, 5], n=2, sc=(-inf, -1.0)), "scores[0]"), (dict(off=[0, 2, 5], n=2, sc=None), "scores"),
                   (dict(off=[0, 2, 5], n=2, us=nan), "unk_score"), (dict(off=[0, 2, 5], n=2, us=-inf), "unk_score"),
                   (dict(off=[0, 2, 5], n=2, mk=b"abcde"), "marker_len"), (dict(off=[0, 2, 5], n=2, ml=-1), "marker_len"),
                   (dict(off=[0, 2, 5], n=2, mk=b"ab"), "one character"), (dict(off=[0, 2, 5], n=2, mk=b"\xc3\xa9a"), "one character"),
                   (dict(off=[0, 2, 5], n=2, out=None), "uni_out"), (dict(off=[0, 2, 5], n=2, w=None), "words")):
    rc = create(**kw)
    assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), (kw, rc, _lib.last_error())
    assert not h.value
assert lib.latok_unigram_info(None, *([None] * 12)) == _lib.ERR_INVALID
assert lib.latok_unigram_destroy(None) == 0
assert create([0, 2, 5], 2) == _lib.ERR_NOT_INIT and not h.value
assert create([0, 2, 5], 2, mk=b"", fu=0, mb=1) == _lib.ERR_NOT_INIT and not h.value
assert create([0, 2, 5], 2, mk=b"\x80\x80") == _lib.ERR_NOT_INIT and not h.value
# the calls: a stray flag bit first, then the missing device; nothing is written
u8, boff = np.frombuffer(b"abc def", np.uint8), np.array([0, 7], np.int64)
ids, ip, n = np.full(8, 0x5A5A5A5A, np.int32), np.full(2, -7, np.int64), C.c_int64(0)
for flags in (4, 64, 1 << 20):
    rc = lib.latok_unigram_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, None, -1, ip.ctypes.data, ids.ctypes.data, None, 8, C.byref(n), None, flags, None)
    assert rc == _lib.ERR_INVALID and "flag" in _lib.last_error(), rc
    rc = lib.latok_unigram_padded_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, None, -1, 8, 1, 1, 2, 0, ids.ctypes.data, ip.ctypes.data, None, flags, None)
    assert rc == _lib.ERR_INVALID and "flag" in _lib.last_error(), rc
rc = lib.latok_unigram_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, None, -1, ip.ctypes.data, ids.ctypes.data, None, 8, C.byref(n), None, 0, None)
assert rc == _lib.ERR_NOT_INIT, rc
assert (ids == 0x5A5A5A5A).all() and (ip == -7).all()
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_the_python_wrappers_refuse_bad_arguments_before_any_device():
    """LATOK_DEVICE names a device no machine has: anything that reached the library's init would raise RuntimeError instead"""
    code = r"""
import sys
sys.path.insert(0, %r)
from latok_amd import batch
for kw in (dict(max_bytes=0), dict(max_bytes=4097), dict(max_bytes=2.5), dict(max_bytes=True), dict(fuse_unk=2), dict(fuse_unk="yes"), dict(seed=-1),
           dict(ids=[1]), dict(ids=[1 << 31, 0]), dict(marker=b"abcde"), dict(marker=b"ab"), dict(marker="ab"), dict(unk_score=float("nan")),
           dict(unk_score=float("-inf")), dict(scores=[-1.0]), dict(scores=[-1.0, float("inf")]), dict(scores=[-1.0, float("nan")])):
    kw.setdefault("scores", [-1.0, -2.0])
    try:
        batch.Unigram([b"a", "b"], **kw)
        raise SystemExit("no ValueError for %%r" %% (kw,))
    except ValueError:
        pass
fake = batch.Unigram.__new__(batch.Unigram)
fake.handle = None
for call in (lambda: batch.unigram_ids_utf8_batch([b"a"], fake), lambda: batch.unigram_ids_batch(["a"], None), lambda: batch.unigram_encode_utf8_batch([b"a"], fake, 8),
             lambda: batch.unigram_ids_utf8_batch([b"a"], batch.BPE.__new__(batch.BPE))):
    try:
        call()
        raise SystemExit("no ValueError for the vocabulary")
    except ValueError as e:
        assert "unigram" in str(e)
for kw in (dict(max_length=0), dict(max_length=2, bos_id=1, eos_id=2), dict(max_length=8, bos_id=1), dict(max_length=8, unk_id=1 << 31),
           dict(max_length=8, pad_id=None)):
    try:
        batch.unigram_encode_utf8_batch([b"a"], fake, **kw)
        raise SystemExit("no ValueError for %%r" %% (kw,))
    except ValueError:
        pass
try:
    batch.Unigram([b"a", "b"], [-1.0, -2.5], ids=[5, -5], seed=7, fuse_unk=False, max_bytes=64, marker="")
    raise SystemExit("no RuntimeError")
except RuntimeError:
    pass
print("ok")
""" % ROOT
    env = dict(os.environ, LATOK_DEVICE="4095")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_from_vocab_file_reads_what_the_test_wrote(tmp_path, monkeypatch):
    from latok_amd import batch
    words = ["<unk>", "▁", "▁the", "s", "é", "日本", "a b"]
    scores = [0.0, -2.5, -3.25, -4.0, -9.125, -11.5, -12.0]
    made = []
    monkeypatch.setattr(batch.Unigram, "__init__", lambda self, w, s, **kw: made.append((list(w), list(s), kw)))
    path = tmp_path / "m.vocab"
    path.write_bytes(b"".join(w.encode() + b"\t" + repr(s).encode() + b"\n" for w, s in zip(words, scores)))
    batch.Unigram.from_vocab_file(str(path), fuse_unk=False, max_bytes=99)
    assert made == [([w.encode() for w in words], scores, dict(fuse_unk=False, max_bytes=99))]
    for bad in (b"a\t-1\nb\n", b"a\t-1\nb\tx\n", b"a\t-1\t2\n"):
        path.write_bytes(bad)
        with pytest.raises(ValueError):
            batch.Unigram.from_vocab_file(str(path))
    assert len(made) == 1
