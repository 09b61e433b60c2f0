"""The cl100k / Llama 3 pre-tokenizer (include/latok_hip.h: LATOK_PRETOK_CL100K), the parts that need no device: the surface (exports,
bindings, header comment, strict C99, argument checks before any device); tests/helpers/pretok_cl100k_ref.py -- a plain restatement of
the definition over bytes -- against the recorded worked table and, where it is installed, against the ``regex`` package; the
contraction letters that (?i) admits, swept over every code point; pretok.h compiled by g++ (once more with the address and
undefined-behaviour sanitizers, as a stand-alone program): the scalar walk AND a CPU model of the device scheme (word records -> tile
records -> the record walk -> the word function, with the tile size and the walk width shrunk so that small inputs cross every level)
against the reference; the tokenizer.json loader."""
import ctypes as C
import json
import os
import random
import re
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT
from helpers import bpe_ref
from helpers import pretok_cl100k_ref as ref
from test_pretok_host import MALFORMED

GEOMETRIES = [(64, 64), (4, 4), (1, 1), (3, 2), (2, 5)]   # (words per tile, tile records per walk step); the device has the first


def worked():
    with open(os.path.join(GOLDEN, "pretok_cl100k_worked.json"), encoding="utf-8") as f:
        return json.load(f)["cases"]


def run_cases(word=64, tile=4096, group=4 * 4096, halo=16, big=True):
    """the runs that exercise the carries, as (name, bytes) -- shared with tests/test_gpu_pretok_cl100k.py.  `big`: also the lengths
    round 64 tiles."""
    lengths = sorted(set(list(range(1, 8)) + list(range(halo - 1, halo + 3)) + list(range(63, 67)) + list(range(127, 131)) +
                         list(range(tile - 1, tile + 3)) + [2 * tile + 1, group - 1, group + 1]))
    if big:
        lengths += [64 * tile - 1, 64 * tile + 1, 64 * tile + tile + 1]
    return lengths


N1, N2, N3, N4 = b"7", "٣".encode(), "३".encode(), "\U0001D7D8".encode()


def run_kinds():
    """name -> f(n): a text whose run has n characters"""
    mixed_n = [N1, N2, N3, N4, N1, N1, N3]
    mixed_s = [b" ", b"\t", "　".encode(), b" ", "\u0085".encode(), b" ", " ".encode()]

    def cyc(units, n):
        reps = n // len(units) + 1
        return b"".join(units * reps)[:sum(len(u) for u in (units * reps)[:n])]

    kinds = {}
    for name, unit in (("N1", N1), ("N2", N2), ("N3", N3), ("N4", N4)):
        kinds[name] = lambda n, u=unit: u * n + b" x"
    kinds["Nmixed"] = lambda n: cyc(mixed_n, n) + b"a"
    kinds["L+N"] = lambda n: b"ab" + N1 * n + b"cd"
    kinds["O+N"] = lambda n: b"!" + N1 * n + b"!"
    kinds["S+N"] = lambda n: b" " + cyc(mixed_n, n)
    kinds["O+NL"] = lambda n: b"a!" + b"\n" * n
    kinds["O+NL+SP"] = lambda n: b"!" + b"\r\n" * (n // 2) + b"\n" * (n % 2) + b" " * (n // 2 + 1)
    kinds["O+NL+SP+NL"] = lambda n: b"?" + b"\n" * n + b" " * n + b"\n"
    kinds["O+NL+text"] = lambda n: b"!" + b"\n" * n + b"text"
    kinds["NL+SP+NL"] = lambda n: b"a\n" + b" " * n + b"\n b"
    kinds["NL+SP+text"] = lambda n: b"\n" + b" " * n + b"text"
    kinds["NL+SP+end"] = lambda n: b"a\n" + b" " * n
    kinds["Smixed"] = lambda n: b"a" + cyc(mixed_s, n) + b"b"
    kinds["longO"] = lambda n: b" !" + b"\x80" * n + b"a b!" + b"\xbf" * n + b"a"
    return kinds


# ---- the surface -----------------------------------------------------------------------------------------------------------
def test_entry_points_header_and_constant():
    from latok_amd import _lib, batch
    _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "latok_amd", "liblatok_hip.so")], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("latok_pretokens_utf8_bytes_batch", "latok_bpe_create_pretok", "latok_bpe_pretokenizer", "latok_debug_pretok_cl100k_limits", "latok_debug_pretok_limits"):
        assert name in exported, name
    for name in ("latok_pretokens_utf8_bytes_batch", "latok_bpe_create_pretok", "latok_bpe_pretokenizer"):
        assert name in _lib.SIGNATURES
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    assert "#define LATOK_PRETOK_CL100K 3" in text and _lib.PRETOK_CL100K == 3
    assert text.index("int latok_bpe_pretokenizer(") < text.index("#define LATOK_PRETOK_CL100K")
    comment = text[:text.index("#define LATOK_PRETOK_CL100K")].rsplit("/*", 1)[1]
    for needle in (ref.PATTERN, "absorbed", "nl_ahead", "U+017F", "reserved", "o200k_base", "add_prefix_space", "flow form", "DevicePool", "max_bytes"):
        assert needle in comment, needle
    assert batch._PRETOKENIZERS["cl100k"] == 3 and batch.BPE.CL100K_PATTERN == ref.PATTERN
    assert callable(batch.BPE.from_tokenizer_json) and callable(batch.BPE.tokenizer_json_word_list)


def test_limits_hook():
    from latok_amd import _lib
    import numpy as np
    lib = _lib.load()
    fn = lib.latok_debug_pretok_cl100k_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(5, np.int64)
    assert fn(out.ctypes.data, 5) == 5
    assert out[0] == 64 and out[1] == 64 * out[0] and out[2] % 64 == 0 and 0 < out[2] <= 1024 and 8 <= out[3] <= out[0] and 1 <= out[4] <= 64
    assert fn(out.ctypes.data, 2) == 2 and fn(None, 5) < 0
    old = lib.latok_debug_pretok_limits
    old.restype, old.argtypes = C.c_int, [C.c_void_p, C.c_int]
    four = np.zeros(5, np.int64)
    assert old(four.ctypes.data, 5) == 4 and (four[:4] == out[:4]).all()


def test_header_is_c99_and_the_example_compiles(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "latok_hip.h"\n'
                   "int f(const uint8_t* u, const int64_t* o, int64_t* cnt, int64_t* sp, int64_t* n) {\n"
                   "    latok_bpe* w = NULL;\n"
                   "    int pt = -1;\n"
                   "    int rc = latok_bpe_create_pretok(u, o, 1, NULL, 4096, 0, LATOK_PRETOK_CL100K, 7u, &w);\n"
                   "    rc += latok_bpe_pretokenizer(w, &pt);\n"
                   "    rc += latok_pretokens_utf8_bytes_batch(u, o, 1, -1, LATOK_PRETOK_CL100K, cnt, sp, 64, n, LATOK_OUT_INT32, NULL);\n"
                   "    return rc + pt + latok_bpe_destroy(w);\n}\n")
    strict = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c"]
    subprocess.check_call(strict + [str(src), "-o", str(tmp_path / "use.o")])
    subprocess.check_call(strict + [os.path.join(ROOT, "examples", "bpe_cl100k_utf8.c"), "-o", str(tmp_path / "example.o")])


def test_the_calls_take_3_and_refuse_bad_arguments_before_they_ask_for_a_device():
    code = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import _lib
lib = _lib.load()
words = np.frombuffer(b"abcde", np.uint8)
off = np.array([0, 2, 5], np.int64)
h = C.c_void_p()
def create(ls=0, pt=3, mb=4096):
    return lib.latok_bpe_create_pretok(words.ctypes.data, off.ctypes.data, 2, None, mb, ls, pt, 0, C.byref(h))
for kw, needle in ((dict(pt=2), "pretok"), (dict(pt=4), "pretok"), (dict(pt=3, ls=1), "lead_space"), (dict(pt=3, mb=0), "max_bytes")):
    rc = create(**kw)
    assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), (kw, rc, _lib.last_error())
    assert not h.value
assert create(pt=3, ls=1) == _lib.ERR_INVALID and "LATOK_PRETOK_CL100K" in _lib.last_error()
assert create() == _lib.ERR_NOT_INIT and not h.value          # pretok = 3 fails only for the missing device
u8, boff = np.frombuffer(b"abc def", np.uint8), np.array([0, 7], np.int64)
cnt, sp, n = np.full(2, -7, np.int64), np.full(16, -7, np.int64), C.c_int64(-3)
def spans(pretok, flags=0):
    return lib.latok_pretokens_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, pretok, cnt.ctypes.data, sp.ctypes.data, 8, C.byref(n), flags, None)
for pretok in (2, 4, -1):
    assert spans(pretok) == _lib.ERR_INVALID and "pretok" in _lib.last_error()
for flags in (4, 64):
    assert spans(3, flags) == _lib.ERR_INVALID and "flag" in _lib.last_error()
assert spans(3) == _lib.ERR_NOT_INIT
assert (cnt == -7).all() and (sp == -7).all() and n.value == -3
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_the_python_wrappers_take_cl100k_and_refuse_cl100k_base_before_any_device():
    """LATOK_DEVICE names a device no machine has: anything that reached the library's init raises RuntimeError instead"""
    code = r"""
import sys
sys.path.insert(0, %r)
from latok_amd import batch
u8, off = batch.pack_utf8([b"a b"])
for call in (lambda: batch.BPE([b"a", "b"], pretokenizer="cl100k_base"), lambda: batch.BPE([b"a", "b"], pretokenizer="cl100k", lead_space=True),
             lambda: batch.pretokens_utf8_csr(u8, off, "cl100k_base"), lambda: batch.pretokenize_utf8_batch([b"a"], pretokenizer="cl100k_base"),
             lambda: batch.pretokenize_batch(["a"], "CL100K")):
    try:
        call()
        raise SystemExit("no ValueError")
    except ValueError:
        pass
assert batch.pretokenize_utf8_batch([], "cl100k") == [] and batch.pretokenize_batch([], "cl100k") == []
for call in (lambda: batch.BPE([b"a", "b"], pretokenizer="cl100k"), lambda: batch.pretokens_utf8_csr(u8, off, "cl100k"),
             lambda: batch.pretokenize_utf8_batch([b"a b"], "cl100k"), lambda: batch.pretokenize_batch(["a b"], "cl100k"),
             lambda: batch.BPE.from_tokenizer_json(%r), lambda: batch.BPE.from_tiktoken_file(%r, pretokenizer="cl100k")):
    try:
        call()
        raise SystemExit("no RuntimeError")
    except RuntimeError:
        pass
print("ok")
""" % (ROOT, os.path.join(GOLDEN, "pretok_cl100k", "tokenizer.json"), "%s")
    import base64
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".tiktoken", delete=False) as f:
        f.write("".join("%s %d\n" % (base64.b64encode(bytes([b])).decode(), b) for b in range(256)))
    try:
        env = dict(os.environ, LATOK_DEVICE="4095")
        out = subprocess.run([sys.executable, "-c", code % f.name], capture_output=True, text=True, env=env, timeout=300)
    finally:
        os.unlink(f.name)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_the_reference_gives_the_worked_table():
    cases = worked()
    assert len(cases) >= 200
    for c in cases:
        b = c["text"].encode()
        assert ref.starts(b) == c["starts"], c["text"]
        spans = ref.pretokens(b)                    # every byte lies in exactly one pre-token
        assert b"".join(b[a:e] for a, e in spans) == b and all(e > a for a, e in spans)
    text = "!\n\n  \n x 1234567  \t!".encode()
    assert [text[a:e] for a, e in ref.pretokens(text)] == [b"!\n\n", b"  \n", b" x", b" ", b"123", b"456", b"7", b"  ", b"\t", b"!"]
    assert [c for c in cases if c["text"] == text.decode()]


def test_the_reference_agrees_with_the_regex_package():
    regex = pytest.importorskip("regex")
    pat = regex.compile(ref.PATTERN)
    rng = random.Random(1)
    for _ in range(200000):
        t = ref.random_text(rng)
        prefix = [0]
        for ch in t:
            prefix.append(prefix[-1] + len(ch.encode()))
        at = [prefix[m.start()] for m in pat.finditer(t)]
        b = t.encode()
        assert ref.starts(b) == at, t
        assert sum(e - a for a, e in ref.pretokens(b)) == len(b)


def test_the_contraction_letters_that_ignore_case_admits():
    """every code point as the one letter, and as either letter of a two-letter contraction, against the ``regex`` package"""
    regex = pytest.importorskip("regex")
    pat = regex.compile(r"(?i:'s|'t|'re|'ve|'m|'ll|'d)")
    one, two = set(), set()
    for cp in range(0x110000):
        if 0xD800 <= cp <= 0xDFFF:
            continue
        ch = chr(cp)
        if pat.fullmatch("'" + ch):
            one.add(ch)
        for other in "rReEvVlL":
            if pat.fullmatch("'" + ch + other) or pat.fullmatch("'" + other + ch):
                two.add(ch)
    assert one == set("DMSTdmst") | {"ſ"} and two == set("rReEvVlL")
    assert sorted(ref.ONE) == sorted(c.encode() for c in one) and {bytes([c]) for w in ref.TWO for c in w} == {c.encode() for c in two}


# ---- pretok.h on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    """the stand-alone program, built by plain g++ and once more with -fsanitize=address,undefined; it is run directly"""
    exe = tmp_path_factory.mktemp("pretok_cl100k_" + request.param) / "pretok_cl100k_harness"
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "pretok_cl100k_harness.cpp"), "-o", str(exe)])

    def run(script):
        out = subprocess.run([str(exe)], input=script, capture_output=True, text=True)
        assert out.returncode == 0, ({3: "the model of the device scheme and the scalar walk disagree"}.get(out.returncode, out.returncode), out.stderr[-2000:])
        return out.stdout.splitlines()

    return run


def _check(harness, batches, geometries=GEOMETRIES):
    """every string of every batch (packed as the device gets it) against the reference, under every geometry"""
    want = {}
    for words_per_tile, step in geometries:
        lines = ["P %d %d" % (words_per_tile, step)]
        for b in batches:
            lines.append("B %d" % len(b))
            lines += [s.hex() or "-" for s in b]
        got = harness("\n".join(lines) + "\n")
        assert len(got) == sum(len(b) for b in batches)
        k = 0
        for b in batches:
            for s in b:
                g = [] if got[k] == "-" else [int(x) for x in got[k].split()]
                if s not in want:
                    want[s] = ref.starts(s)
                assert g == want[s], ((words_per_tile, step), s[:200], g[:50], want[s][:50])
                k += 1


def test_the_worked_table(harness):
    blobs = [c["text"].encode() for c in worked()]
    _check(harness, [[b] for b in blobs] + [blobs, blobs[::-1], [b"", b""] + blobs[:40] + [b""]])


def test_random_text(harness):
    rng = random.Random(5)
    batches, n = [], 0
    while n < 8000:
        batches.append([ref.random_text(rng, 60).encode() for _ in range(rng.randint(1, 40))])
        n += len(batches[-1])
    _check(harness, batches)


def test_malformed_bytes(harness):
    rng = random.Random(6)
    fixed = [[b"a\xe3", b"\x80\x80b"], [b"\xf0\x9f", b"\xa4\x93"], [b"it'", b"s"], [b"it'l", b"l"], [b"it'\xc5", b"\xbf"], [b" ", b"a"], [b"\xe3\x80", b"\x80"], [b"\xc2"],
             [b"\x80"], [b"\xff" * 70], [b"\x80" * 130], [b"\xe3" + b"\x80" * 66 + b"a"], [b"!" + b"\xe3" + b"\x80" * 66 + b"a"], [b" !" + b"\x80" * 300 + b"a"],
             [b"b!" + b"\x80" * 300 + b"a"], [b"!\n\x80", b"1\x80" * 5 + b"1111"]]
    _check(harness, fixed)
    pieces = MALFORMED + [b"\n", b"\r", b"!", b"'\xc5\xbf", b"'S", b"'Re", b"7", b"\xd9\xa3"]
    _check(harness, [[b"".join(rng.choice(pieces) for _ in range(rng.randint(0, 24))) for _ in range(rng.randint(1, 40))] for _ in range(250)])
    _check(harness, [[bytes(rng.randrange(256) for _ in range(rng.randint(0, 200))) for _ in range(10)] for _ in range(100)])


FEATURES = [b"a's b", b"we'LL go", b"x'Re", b"it'\xc5\xbf x", b"x 's", b"!'s", b"\t's", b"a!b", b"a\tb", b"a b", b"a !b", b" !", b"!!a", b"!a", b"a\n\nb", b"a \n b",
            b"!\n\n a", b"! \n", b"a\r\n\r\nb", b"\n  x", b"\n  \n", b"a  b", b"a\xe3\x80\x80\xe3\x80\x80b", b"a\xe3\x80\x80 b", b"1234567", b"a12b", b" 1",
            b"\xf0\x9d\x9f\x98\xf0\x9d\x9f\x98\xf0\x9d\x9f\x98\xf0\x9d\x9f\x98", b"\xf0\x9d\x9f\x98\xf0\x9f\xa4\x93", b"a\xe3\x80\x80's"]


def test_every_feature_at_every_offset_across_a_word_edge(harness):
    batches = []
    for f in FEATURES:
        for pad in range(64 - len(f) - 2, 66):
            batches.append([b"x" * pad + f])
            for cut in range(1, len(f)):
                batches.append([b"y" * pad + f[:cut], f[cut:] + b" z"])
    _check(harness, batches, GEOMETRIES[:3])


def test_the_runs_that_the_carries_cross(harness):
    """every kind of run at every length up to a little over two (shrunk) tiles and every start offset, whole, with a string boundary
    inside the run, and cut by the batch's end"""
    kinds = run_kinds()
    lengths = [n for n in run_cases(big=False) if n <= 131] + [255, 257, 300, 513, 700]
    batches = []
    for name, make in kinds.items():
        for n in lengths:
            text = make(n)
            for offset in range(12) if n <= 66 else range(4):
                pad = b"x " * 32
                lead = pad[:64 - offset] if offset else b""
                batches.append([lead + text])
                batches.append([lead + text[:len(text) // 2], text[len(text) // 2:]])         # a string boundary inside the run
                batches.append([lead + text[:len(text) // 2 + 1]])                             # the batch's end cuts the run
    _check(harness, batches, GEOMETRIES[1:4])
    _check(harness, [[b"", b""] + [b[0] for b in batches[:300]] + [b""]], GEOMETRIES[:2])


# ---- the tokenizer.json loader -----------------------------------------------------------------------------------------------
def test_from_tokenizer_json(tmp_path, monkeypatch):
    from latok_amd import batch
    path = os.path.join(GOLDEN, "pretok_cl100k", "tokenizer.json")
    tj = json.load(open(path, encoding="utf-8"))
    words, ids, specials, name = batch.BPE.tokenizer_json_word_list(path)
    vocab = tj["model"]["vocab"]
    dec = batch.BPE.gpt2_byte_decoder()
    enc = {v: k for k, v in dec.items()}
    assert name == "cl100k" and specials == {"<|end_of_text|>": 0} and words[:256] == [bytes([b]) for b in range(256)] and len(words) == len(vocab) - 1
    merges = [m.split(" ") if isinstance(m, str) else m for m in tj["model"]["merges"]]
    assert [bytes(dec[c] for c in a + b) for a, b in merges] == words[256:]
    assert ids == [vocab["".join(enc[x] for x in w)] for w in words]
    # the recorded ids, by the two references over this word list (what the device call is held to on the GPU)
    d = bpe_ref.rank_dict(words)
    cases = json.load(open(os.path.join(GOLDEN, "pretok_cl100k_cases.json"), encoding="utf-8"))["cases"]
    assert len(cases) >= 200
    for c in cases:
        blob = c["text"].encode()
        got = [pid for a, e in ref.pretokens(blob) for pid, _, _ in bpe_ref.cut(blob[a:e], d, 4096, -1, ids)]
        assert got == c["ids"], c["text"]
    # the constructor gets the list, the ids and the detected pre-tokenizer; the specials land on the object
    made = []
    monkeypatch.setattr(batch.BPE, "__init__", lambda self, w, **kw: made.append((list(w), kw)))
    obj = batch.BPE.from_tokenizer_json(path, max_bytes=99)
    assert made == [(words, dict(ids=ids, pretokenizer="cl100k", max_bytes=99))] and obj.specials == specials

    def variant(name, change):
        doc = json.loads(json.dumps(tj))
        change(doc)
        p = tmp_path / (name + ".json")
        p.write_text(json.dumps(doc), encoding="utf-8")
        return str(p)

    # merges as pairs; a GPT-2-style file
    as_pairs = variant("pairs", lambda d: d["model"].__setitem__("merges", [m.split(" ") if isinstance(m, str) else " ".join(m) for m in d["model"]["merges"]]))
    assert batch.BPE.tokenizer_json_word_list(as_pairs) == (words, ids, specials, "cl100k")
    gpt2 = variant("gpt2", lambda d: d.__setitem__("pre_tokenizer", {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True}))
    assert batch.BPE.tokenizer_json_word_list(gpt2) == (words, ids, specials, "gpt2")
    batch.BPE.from_tokenizer_json(gpt2, pretokenizer="latok", lead_space=True)
    assert made[1][1] == dict(ids=ids, pretokenizer="latok", lead_space=True)
    seq = lambda d: d["pre_tokenizer"]["pretokenizers"]   # noqa: E731
    refused = {
        "another pattern": lambda d: seq(d)[0]["pattern"].__setitem__("Regex", r"\s+"),
        "a string pattern": lambda d: seq(d)[0].__setitem__("pattern", {"String": " "}),
        "inverted": lambda d: seq(d)[0].__setitem__("invert", True),
        "not isolated": lambda d: seq(d)[0].__setitem__("behavior", "Removed"),
        "ByteLevel with its regex behind the split": lambda d: seq(d)[1].__setitem__("use_regex", True),
        "add_prefix_space": lambda d: seq(d)[1].__setitem__("add_prefix_space", True),
        "three steps": lambda d: seq(d).append({"type": "Digits", "individual_digits": True}),
        "ByteLevel without its regex alone": lambda d: d.__setitem__("pre_tokenizer", {"type": "ByteLevel", "add_prefix_space": False, "use_regex": False}),
        "gpt2 add_prefix_space": lambda d: d.__setitem__("pre_tokenizer", {"type": "ByteLevel", "add_prefix_space": True, "use_regex": True}),
        "whitespace": lambda d: d.__setitem__("pre_tokenizer", {"type": "Whitespace"}),
        "none": lambda d: d.__setitem__("pre_tokenizer", None),
        "a normalizer": lambda d: d.__setitem__("normalizer", {"type": "NFC"}),
        "another model": lambda d: d["model"].__setitem__("type", "WordPiece"),
        "a merge that is no pair": lambda d: d["model"]["merges"].__setitem__(3, "a b c"),
        "a merge result the vocab lacks": lambda d: d["model"]["vocab"].pop("".join(merges[5])),
    }
    for what, change in refused.items():
        with pytest.raises(ValueError, match="tokenizer.json"):
            batch.BPE.tokenizer_json_word_list(variant("bad", change))
    assert len(made) == 2
    # gpt2_word_list keeps its behaviour
    model = os.path.join(GOLDEN, "pretok_gpt2")
    w2, i2, s2 = batch.BPE.gpt2_word_list(os.path.join(model, "vocab.json"), os.path.join(model, "merges.txt"))
    assert w2[:256] == [bytes([b]) for b in range(256)] and s2 == {"<|endoftext|>": 0} and len(i2) == len(w2)
