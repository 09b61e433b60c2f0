"""SentencePiece BPE (include/latok_hip.h: LATOK_PRETOK_SPM, latok_bpe_create_spm), the parts that need no device: the surface
(exports, bindings, header comment, strict C99, argument checks before any device); tests/helpers/spbpe_ref.py -- a plain restatement
of the definition over bytes -- against the hand-worked segment tables, the recorded ``sentencepiece`` and ``tokenizers`` ids and, where
it is installed, the ``sentencepiece`` package itself; spbpe.h compiled by g++ (once more with the address and undefined-behaviour
sanitizers, as a stand-alone program): the scalar and the plane form of the segment rule, the virtual text, and bpe_merge on the lane
state and on a wide state, against the reference on random strings; the two loaders and each of their refusals."""
import ctypes as C
import json
import os
import random
import shutil
import struct
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT
from helpers import spbpe_ref as ref

DIR = os.path.join(GOLDEN, "spbpe")
MODEL, TOKJSON = os.path.join(DIR, "m.model"), os.path.join(DIR, "tokenizer.json")
MARK = ref.MARK
UNK = -7
EDGE = [b"", b" ", b"a  b", b"a" + MARK + b" b", b"  ", MARK, MARK + MARK, b"a", b" a", b"a ", b"\t", b"a\tb c", b"\xe2\x96", b"a \xe2\x96", b"\xe2\x96\x81\x80",
        b" \x80", b"\x80", b"\x80\x80 a", b"\xe2", b"a\xf0\x9f", b"\xf0\x9f\x98\x80", b" " * 70, MARK * 30, b"a" * 70, b" " * 21 + b"a", b" " * 20 + b"abcd",
        (b" " + MARK) * 12 + b"xyz", b"ab" * 40 + b" " + b"cd" * 40, "日本語".encode() * 30]


def cases():
    with open(os.path.join(DIR, "spbpe_cases.json"), encoding="utf-8") as f:
        return json.load(f)["cases"]


def model_lists():
    from latok_amd.batch import BPE
    return BPE.sentencepiece_word_list(MODEL)


# ---- the surface -----------------------------------------------------------------------------------------------------------
def test_entry_points_header_and_constant():
    from latok_amd import _lib, batch
    _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "latok_amd", "liblatok_hip.so")], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("latok_bpe_create_spm", "latok_bpe_spm_info", "latok_debug_spbpe_limits"):
        assert name in exported, name
    for name in ("latok_bpe_create_spm", "latok_bpe_spm_info"):
        assert name in _lib.SIGNATURES
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    assert "#define LATOK_PRETOK_SPM 5" in text and _lib.PRETOK_SPM == 5 and batch._PRETOKENIZERS["spm"] == 5
    comment = text[:text.index("#define LATOK_PRETOK_SPM")].rsplit("/*", 1)[1]
    for needle in ("E2 96 81", "SPACE-LIKE", "VIRTUAL TEXT", "no whole-segment shortcut", "byte_ids[b]", "fuse_unk", "empty range", "reserved",
                   # what is out of scope
                   "NFKC", "USER_DEFINED", "decoder mode", "BOS-only", "special-token strings", "flow form", "folding inside the call", "DevicePool"):
        assert needle in comment, needle
    for name in ("sentencepiece", "from_sentencepiece_model", "sentencepiece_word_list", "from_spm_tokenizer_json", "spm_tokenizer_json_word_list"):
        assert callable(getattr(batch.BPE, name))


def test_limits_hook():
    import numpy as np
    from latok_amd import _lib
    lib = _lib.load()
    fn = lib.latok_debug_spbpe_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(4, np.int64)
    assert fn(out.ctypes.data, 4) == 3
    assert out[0] % 64 == 0 and 0 < out[0] <= 1024 and out[1] == 64 and out[2] == 4096
    assert fn(out.ctypes.data, 2) == 2 and fn(None, 3) < 0


def test_header_is_c99_and_the_example_compiles(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "latok_hip.h"\n'
                   "int f(const uint8_t* u, const int64_t* o, const int32_t* by, int64_t* cnt, int64_t* sp, int64_t* n) {\n"
                   "    latok_bpe* w = NULL;\n"
                   "    int pt = -1, a = 0, b = 0, c = 0;\n"
                   "    int rc = latok_bpe_create_spm(u, o, 1, NULL, by, 1, 0, 4096, 7u, &w);\n"
                   "    rc += latok_bpe_pretokenizer(w, &pt) + latok_bpe_spm_info(w, &a, &b, &c);\n"
                   "    rc += latok_pretokens_utf8_bytes_batch(u, o, 1, -1, LATOK_PRETOK_SPM, cnt, sp, 64, n, LATOK_OUT_INT32, NULL);\n"
                   "    return rc + pt + a + b + c + latok_bpe_destroy(w);\n}\n")
    strict = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c"]
    subprocess.check_call(strict + [str(src), "-o", str(tmp_path / "use.o")])
    subprocess.check_call(strict + [os.path.join(ROOT, "examples", "spbpe_utf8.c"), "-o", str(tmp_path / "example.o")])


def test_the_calls_take_5_and_refuse_bad_arguments_before_they_ask_for_a_device():
    code = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import _lib
lib = _lib.load()
words = np.frombuffer(b"ab\xe2\x96\x81cde", np.uint8)
off = np.array([0, 2, 6, 8], np.int64)            # ab, <marker>c, de
by = np.arange(256, dtype=np.int32)
h = C.c_void_p()
def create(w=words, o=off, n=3, by=by, dummy=1, fuse=0, mb=4096):
    return lib.latok_bpe_create_spm(w.ctypes.data, o.ctypes.data, n, None, by.ctypes.data if by is not None else None, dummy, fuse, mb, 0, C.byref(h))
for kw, needle in ((dict(dummy=2), "add_dummy_prefix"), (dict(dummy=-1), "add_dummy_prefix"), (dict(fuse=2), "fuse_unk"), (dict(mb=0), "max_bytes"),
                   (dict(mb=4097), "max_bytes"), (dict(o=np.array([0, 2, 1, 8], np.int64)), "")):
    rc = create(**kw)
    assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), (kw, rc, _lib.last_error())
    assert not h.value
bad = np.frombuffer(b"abc\xe2\x96\x81\xe2\x96\x81\xe2\x96\x81x", np.uint8)   # ab, c<marker>, <marker><marker>x: word 1 breaks the rule
assert create(w=bad, o=np.array([0, 2, 6, 13], np.int64)) == _lib.ERR_INVALID and "word 1 " in _lib.last_error(), _lib.last_error()
assert lib.latok_bpe_create_spm(words.ctypes.data, off.ctypes.data, 3, None, None, 1, 0, 4096, 0, None) == _lib.ERR_INVALID
assert create() == _lib.ERR_NOT_INIT and not h.value          # a fine list fails only for the missing device
assert create(by=None, fuse=1) == _lib.ERR_NOT_INIT and not h.value
# latok_bpe_create_pretok goes on refusing 5 (and 2 and 4)
for pt in (5, 2, 4):
    rc = lib.latok_bpe_create_pretok(words.ctypes.data, off.ctypes.data, 3, None, 4096, 0, pt, 0, C.byref(h))
    assert rc == _lib.ERR_INVALID and not h.value and ("pretok" in _lib.last_error() or "LATOK_PRETOK_SPM" in _lib.last_error())
a = b = c = C.c_int(0)
assert lib.latok_bpe_spm_info(None, C.byref(a), C.byref(b), C.byref(c)) == _lib.ERR_INVALID
u8, boff = np.frombuffer(b"abc def", np.uint8), np.array([0, 7], np.int64)
cnt, sp, n = np.full(2, -7, np.int64), np.full(16, -7, np.int64), C.c_int64(-3)
def spans(pretok, flags=0):
    return lib.latok_pretokens_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, pretok, cnt.ctypes.data, sp.ctypes.data, 8, C.byref(n), flags, None)
for pretok in (2, 4, 6, -1):
    assert spans(pretok) == _lib.ERR_INVALID and "pretok" in _lib.last_error()
for flags in (4, 64):
    assert spans(5, flags) == _lib.ERR_INVALID and "flag" in _lib.last_error()
assert spans(5) == _lib.ERR_NOT_INIT
assert (cnt == -7).all() and (sp == -7).all() and n.value == -3
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_the_python_wrappers_take_spm_and_refuse_before_any_device():
    """LATOK_DEVICE names a device no machine has: anything that reached the library's init raises RuntimeError instead"""
    code = r"""
import sys
sys.path.insert(0, %r)
from latok_amd import batch
u8, off = batch.pack_utf8([b"a b"])
for call in (lambda: batch.BPE([b"a", "b"], pretokenizer="spm"), lambda: batch.BPE.sentencepiece([b"a"], byte_ids=[1, 2, 3]),
             lambda: batch.BPE.sentencepiece([b"a"], max_bytes=0), lambda: batch.BPE.sentencepiece([b"a"], fuse_unk=2),
             lambda: batch.pretokenize_batch(["a"], "SPM")):
    try:
        call()
        raise SystemExit("no ValueError")
    except ValueError:
        pass
assert batch.pretokenize_utf8_batch([], "spm") == [] and batch.pretokenize_batch([], "spm") == []
for call in (lambda: batch.BPE.sentencepiece([b"a", "b"]), lambda: batch.pretokens_utf8_csr(u8, off, "spm"), lambda: batch.pretokenize_batch(["a b"], "spm"),
             lambda: batch.BPE.from_sentencepiece_model(%r), lambda: batch.BPE.from_spm_tokenizer_json(%r)):
    try:
        call()
        raise SystemExit("no RuntimeError")
    except RuntimeError:
        pass
print("ok")
""" % (ROOT, MODEL, TOKJSON)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, LATOK_DEVICE="4095"), timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_the_reference_gives_the_worked_segment_tables():
    with open(os.path.join(DIR, "spbpe_worked.json"), encoding="utf-8") as f:
        worked = json.load(f)["cases"]
    assert len(worked) >= 16
    for c in worked:
        b = c["text"].encode()
        assert [b[a:e].decode() for a, e in ref.segments(b)] == c["segments"], c["text"]
        assert "".join(c["segments"]) == c["text"]
    assert ref.segments(b"") == [] and ref.segments(b"\xe2\x96\x81\x80 x") == [(0, 4), (4, 6)] and ref.segments(b"a \xe2\x96") == [(0, 1), (1, 4)]


def test_the_reference_gives_the_recorded_ids_of_both_packages():
    words, ids, byte_ids, specials, dummy = model_lists()
    d = ref.rank_dict(words)
    assert dummy and len(byte_ids) == 256 and set(specials) == {"<unk>", "<s>", "</s>"} and ref.bad_word(words) == -1
    all_cases = cases()
    assert len(all_cases) >= 200
    for c in all_cases:          # no case is skipped
        b = c["text"].encode()
        assert all(sum(len(ch) for ch, _, _ in ref.virtual(b[a:e], a == 0)) <= 4096 for a, e in ref.segments(b))
        got, spans = ref.encode(b, d, byte_ids=byte_ids, ids=ids)
        assert got == c["sp_ids"] == c["hf_ids"], c["text"]
        assert len(spans) == len(got) and all(0 <= a <= e <= len(b) for a, e in spans)
        assert [s for s in spans if s[0] < s[1]] == sorted(s for s in spans if s[0] < s[1])


def test_the_reference_spans_are_the_offsets_tokenizers_gave():
    """in characters, for every piece that is not the dummy marker's own (tokenizers gives that one the first character's range)"""
    words, ids, byte_ids, _, _ = model_lists()
    d = ref.rank_dict(words)
    for c in cases():
        b = c["text"].encode()
        at = {}
        for i, ch in enumerate(c["text"]):
            at[len(c["text"][:i].encode())] = i
        at[len(b)] = len(c["text"])
        _, spans = ref.encode(b, d, byte_ids=byte_ids, ids=ids)
        mine = [(at[a], at[e]) for a, e in spans]
        theirs = [tuple(o) for o in c["hf_offsets"]]
        assert len(mine) == len(theirs)
        for m, t in zip(mine, theirs):
            assert m == t or m[0] == m[1] == 0, (c["text"], mine, theirs)


def test_the_reference_agrees_with_the_sentencepiece_package():
    spm = pytest.importorskip("sentencepiece")
    sp = spm.SentencePieceProcessor(model_file=MODEL)
    words, ids, byte_ids, _, _ = model_lists()
    d = ref.rank_dict(words)
    rng = random.Random(3)
    alphabet = list("abcdehlnorstwxyz") + [" "] * 6 + ["  ", "\t", "\n", "é", "日", "€", "😀", "▁", "п"]
    for _ in range(5000):
        t = "".join(rng.choice(alphabet) for _ in range(rng.randint(0, 30)))
        assert ref.encode(t.encode(), d, byte_ids=byte_ids, ids=ids)[0] == [int(i) for i in sp.encode(t)], t


# ---- spbpe.h on the host ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    """the stand-alone program, built by plain g++ and once more with -fsanitize=address,undefined; it is run directly"""
    exe = tmp_path_factory.mktemp("spbpe_" + request.param) / "spbpe_harness"
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "spbpe_harness.cpp"), "-o", str(exe)])

    def run(script):
        out = subprocess.run([str(exe)], input=script, capture_output=True, text=True)
        assert out.returncode == 0, ({2: "a text load left the segment's dwords", 3: "a table load left the table", 4: "the lane state and the wide state disagree",
                                      5: "the plane form of the segment rule disagrees with the scalar walk",
                                      6: "a piece count disagrees with the pieces"}.get(out.returncode, out.returncode), out.stderr[-2000:])
        return out.stdout.splitlines()

    run.sanitized = request.param == "sanitized"
    return run


def _hex(b):
    return b.hex() if b else "-"


def _check(harness, words, texts, ids=None, byte_ids=None, dummy=True, fuse=False, max_bytes=4096, seed=0, pads=(0, 1, 2, 3)):
    d = ref.rank_dict(words)
    script = ["V %x %d %d %d %d" % (seed, max_bytes, dummy, fuse, len(words))]
    script += ["%s %s" % ("-" if ids is None else ids[i], _hex(w)) for i, w in enumerate(words)]
    script.append("Y " + ("-" if byte_ids is None else ",".join(str(i) for i in byte_ids)))
    script += ["E %d %d %s" % (pads[k % len(pads)], UNK, _hex(t)) for k, t in enumerate(texts)]
    lines = harness("\n".join(script) + "\n")
    assert len(lines) == 1 + len(texts)
    for t, line in zip(texts, lines[1:]):
        fields = line.split()
        starts = "" if fields[0] == "-" else fields[0]
        assert [i for i, c in enumerate(starts) if c == "1"] == [a for a, _ in ref.segments(t)], t
        want_ids, want_spans = ref.encode(t, d, byte_ids=byte_ids, add_dummy_prefix=dummy, fuse_unk=fuse, max_bytes=max_bytes, unk=UNK, ids=ids)
        got = [tuple(int(x) for x in f.split(":")) for f in fields[2:]]
        assert int(fields[1]) == len(got)
        assert got == [(i, a, e) for i, (a, e) in zip(want_ids, want_spans)], (t, dummy, fuse, max_bytes)


UNITS = [b"a", b"b", b"c", b"d", b"e", b"t", b"h", b"o", b"l", b"x"] + [b" "] * 6 + [b"  ", MARK, b"\t", b"\n", "é".encode(), "日".encode(), "€".encode(),
                                                                                  "😀".encode(), "п".encode(), b"\x80", b"\xe2\x96", b"\xe2", b"\xf0\x9f", b"\xff"]


def random_texts(rng, n, longest=24):
    return [b"".join(rng.choice(UNITS) for _ in range(rng.randint(0, longest))) for _ in range(n)]


def test_spbpe_h_against_the_reference_on_random_strings(harness):
    """the model's word list with byte fallback, and crafted lists without it, fused and not, with and without the dummy prefix: at least
    100 000 random strings through the plain build (a fifth of them through the sanitized one), malformed bytes included"""
    words, ids, byte_ids, _, _ = model_lists()
    rng = random.Random(11)
    n = 4000 if harness.sanitized else 20000
    _check(harness, words, EDGE + random_texts(rng, 3 * n), ids=ids, byte_ids=byte_ids)
    _check(harness, words, EDGE + random_texts(rng, n), ids=ids, byte_ids=byte_ids, dummy=False)
    small = [b"a", b"b", b"c", MARK, b"ab", MARK + b"a", MARK + MARK, b"abc", MARK + b"ab", "é".encode(), b"t", b"h", b"th", b"the", MARK + b"the"]
    _check(harness, small, EDGE + random_texts(rng, n), dummy=True, fuse=True)
    _check(harness, small, EDGE + random_texts(rng, n), dummy=False, fuse=False, max_bytes=8)
    _check(harness, small, EDGE + random_texts(rng, n // 2, 90), byte_ids=list(range(1000, 1256)), max_bytes=64)
    _check(harness, small, EDGE + random_texts(rng, n // 2, 200), fuse=True, max_bytes=4096, seed=0xdeadbeef)


def test_spbpe_h_virtual_lengths_round_the_lane_limit_and_max_bytes(harness):
    """virtual lengths 1 .. 4 and 62 .. 66 reached by real bytes and by marker expansion; max_bytes - 1 .. max_bytes + 1 for 8 and 4096;
    a lead run that alone passes 64 bytes; every start alignment"""
    small = [b"a", b"b", MARK, b"ab", MARK + b"a", MARK + MARK, MARK + MARK + MARK + MARK, b"abab"]
    texts = []
    for L in list(range(1, 5)) + list(range(62, 67)):
        texts += [b"ab" * (L // 2) + b"a" * (L % 2)]                                       # no dummy: the real bytes alone
        if L >= 4:
            texts += [b"x " + b"ab" * ((L - 3) // 2) + b"a" * ((L - 3) % 2)]               # one space: 3 + (L - 3)
        if L >= 62:
            texts += [b"  " + b"a" * (L - 9), b"q" + b" " * 21 + b"a" * (L - 63) if L >= 63 else b"q"]
    for mb, fuse in ((8, False), (4096, True)):
        for L in (mb - 1, mb, mb + 1):
            texts += [b"ab" * (L // 2) + b"a" * (L % 2), b"z " + b"a" * (L - 3), b"z" + b" " * (L // 3) + b"a" * (L % 3)]
        _check(harness, small, texts, dummy=False, fuse=fuse, max_bytes=mb)
        _check(harness, small, texts, dummy=True, byte_ids=list(range(300, 556)), max_bytes=mb)
    _check(harness, small, [b" " * 30 + b"ab", MARK * 22 + b"ab", (b" " + MARK) * 40 + b"abab", b"a" + b" " * 1365, b"a" + b" " * 1366], byte_ids=list(range(256)))


def test_no_shortcut_and_ranks(harness):
    """abc without ab and bc is never reached; the leftmost of equal ranks; rank beats position"""
    d = ref.rank_dict([b"a", b"b", b"c", b"abc"])
    assert [i for i, _, _ in ref.cut(b"abc", d, add_dummy_prefix=False)] == [0, 1, 2]
    _check(harness, [b"a", b"b", b"c", b"abc"], [b"abc", b"abc abc"], dummy=False)
    words = [b"a", b"b", b"ab", b"ab", b"ba", b"aba"]          # (the second ab is a duplicate: the first wins)
    assert [(a, e) for _, a, e in ref.cut(b"ababab", ref.rank_dict(words), add_dummy_prefix=False)] == [(0, 2), (2, 4), (4, 6)]
    words2 = [b"a", b"b", b"c", b"bc", b"ab"]                  # bc outranks ab: a bc, not ab c
    assert [(a, e) for _, a, e in ref.cut(b"abc", ref.rank_dict(words2), add_dummy_prefix=False)] == [(0, 1), (1, 3)]
    _check(harness, words, [b"ababab", b"bababa", b"aabab b"], dummy=False)
    _check(harness, words2, [b"abc", b"abcabc", b"ababc"], dummy=False)


def test_the_word_list_check(harness):
    for words, want in (([b"a", MARK + b"a", MARK + MARK], -1), ([b"a", b"a" + MARK], 1), ([MARK + b"a" + MARK + b"b"], 0), ([b" " + MARK], 0),
                        ([MARK + MARK + b"ab", b"\x80" + MARK], 1), ([], -1)):
        assert ref.bad_word(words) == want
        script = "V 0 4096 1 0 %d\n" % len(words) + "".join("- %s\n" % _hex(w) for w in words) + "W\n"
        assert harness(script)[-1] == str(want)


# ---- the loaders -----------------------------------------------------------------------------------------------------------
def test_the_two_files_give_the_same_ids_on_every_case():
    from latok_amd.batch import BPE
    words, ids, byte_ids, specials, dummy = model_lists()
    jw, jids, jbytes, jspecials, jdummy = BPE.spm_tokenizer_json_word_list(TOKJSON)
    assert byte_ids == jbytes and dummy == jdummy and specials == jspecials and sorted(zip(words, ids)) == sorted(zip(jw, jids))
    d, jd = ref.rank_dict(words), ref.rank_dict(jw)
    for c in cases():
        b = c["text"].encode()
        assert ref.encode(b, d, byte_ids=byte_ids, ids=ids) == ref.encode(b, jd, byte_ids=jbytes, ids=jids), c["text"]
    m = BPE.read_sentencepiece_model(MODEL)
    assert m["model_type"] == 2 and m["byte_fallback"] and m["normalizer_name"] == "identity" and m["charsmap"] == b"" and m["add_dummy_prefix"]
    assert not m["remove_extra_whitespaces"] and m["escape_whitespaces"] and not m["treat_whitespace_as_suffix"] and len(m["pieces"]) == 400
    scores = [s for _, s, k in m["pieces"] if k == 1]
    assert [w for w in words] == [p for p, _, k in sorted((x for x in m["pieces"] if x[2] == 1), key=lambda x: -x[1])] and scores


def _varint(v):
    out = bytearray()
    while True:
        out.append((v & 0x7F) | (0x80 if v > 0x7F else 0))
        v >>= 7
        if not v:
            return bytes(out)


def _field(no, payload):
    return _varint(no << 3 | 2) + _varint(len(payload)) + payload


def _flag(no, v):
    return _varint(no << 3) + _varint(int(v))


def _model(pieces, model_type=2, byte_fallback=True, suffix=False, name=b"identity", charsmap=b"", dummy=True, remove=False, escape=True):
    out = b""
    for piece, score, kind in pieces:
        out += _field(1, _field(1, piece) + _varint(2 << 3 | 5) + struct.pack("<f", score) + _flag(3, kind))
    out += _field(2, _flag(3, model_type) + _flag(35, byte_fallback) + _flag(24, suffix))
    return out + _field(3, _field(1, name) + (_field(2, charsmap) if charsmap else b"") + _flag(3, dummy) + _flag(4, remove) + _flag(5, escape))


def test_the_model_loader_names_what_it_refuses(tmp_path):
    from latok_amd.batch import BPE
    base = [(b"<unk>", 0.0, 2), (b"<s>", 0.0, 3)] + [(b"<0x%02X>" % b, 0.0, 6) for b in range(256)] + [(MARK + b"a", -1.0, 1), (b"a", -2.0, 1), (MARK, -2.0, 1)]

    def load(**kw):
        pieces = kw.pop("pieces", base)
        p = tmp_path / "x.model"
        p.write_bytes(_model(pieces, **kw))
        return BPE.sentencepiece_word_list(str(p))

    words, ids, byte_ids, specials, dummy = load()
    assert words == [MARK + b"a", b"a", MARK] and ids == [258, 259, 260] and byte_ids == list(range(2, 258)) and specials == {"<unk>": 0, "<s>": 1} and dummy
    assert load(dummy=False)[4] is False and load(byte_fallback=False, pieces=base[:2] + base[258:])[2] is None
    for kw, needle in ((dict(model_type=1), "UNIGRAM"), (dict(name=b"nmt_nfkc"), "nmt_nfkc"), (dict(charsmap=b"\x01\x02"), "charsmap"),
                       (dict(remove=True), "remove_extra_whitespaces"), (dict(escape=False), "escape_whitespaces"), (dict(suffix=True), "treat_whitespace_as_suffix"),
                       (dict(pieces=base + [(b"<user>", 0.0, 4)]), "USER_DEFINED"), (dict(pieces=base + [(b"<unused>", 0.0, 5)]), "UNUSED"),
                       (dict(pieces=base[:200] + base[258:]), "256 byte pieces")):
        with pytest.raises(ValueError, match=needle):
            load(**kw)
    (tmp_path / "junk.model").write_bytes(b"\xff\xff\xff\xff\xff\xff\xff\xff\xff\xff\xff\xff")
    with pytest.raises(ValueError, match="SentencePiece model"):
        BPE.sentencepiece_word_list(str(tmp_path / "junk.model"))


def test_the_tokenizer_json_loader_names_what_it_refuses(tmp_path):
    from latok_amd.batch import BPE
    with open(TOKJSON, encoding="utf-8") as f:
        good = json.load(f)

    def load(edit):
        tj = json.loads(json.dumps(good))
        edit(tj)
        p = tmp_path / "t.json"
        p.write_text(json.dumps(tj), encoding="utf-8")
        return BPE.spm_tokenizer_json_word_list(str(p))

    assert load(lambda tj: tj.update(normalizer=tj["normalizer"]["normalizers"][1]))[4] is False       # the Replace alone: no dummy prefix
    for edit, needle in ((lambda tj: tj["model"].update(byte_fallback=False), "byte_fallback"), (lambda tj: tj["model"].update(type="Unigram"), "not BPE"),
                         (lambda tj: tj.update(pre_tokenizer={"type": "Metaspace"}), "pre_tokenizer"), (lambda tj: tj.update(normalizer=None), "normalizer"),
                         (lambda tj: tj.update(normalizer={"type": "NFKC"}), "normalizer"),
                         (lambda tj: tj["normalizer"]["normalizers"].reverse(), "normalizer"),
                         (lambda tj: tj["normalizer"]["normalizers"][0].update(prepend="_"), "normalizer"),
                         (lambda tj: tj["model"].update(dropout=0.1), "dropout"), (lambda tj: tj["model"].update(ignore_merges=True), "ignore_merges"),
                         (lambda tj: tj["model"]["merges"].append(["zz", "qq"]), "merge result"), (lambda tj: tj["model"]["vocab"].pop("<0x41>"), "255 of the 256"),
                         (lambda tj: tj["model"]["merges"].append("a b c"), "left right")):
        with pytest.raises(ValueError, match=needle):
            load(edit)
    # from_tokenizer_json still refuses the file, and names the reason
    with pytest.raises(ValueError, match="byte_fallback"):
        BPE.tokenizer_json_word_list(TOKJSON)
    with pytest.raises(ValueError):
        BPE.from_tokenizer_json(TOKJSON)


def test_the_fixture_tool_is_seeded():
    """the tool generates its corpus and its texts from fixed seeds and names the fixtures this suite reads"""
    src = open(os.path.join(ROOT, "tools", "make_spbpe_golden.py"), encoding="utf-8").read()
    for needle in ("random.Random(", "m.model", "tokenizer.json", "spbpe_cases.json", "spbpe_worked.json", "byte_fallback=True", 'normalization_rule_name="identity"'):
        assert needle in src, needle
    assert shutil.which("g++")
