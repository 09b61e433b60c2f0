"""GPT-2's pre-tokenizer (include/latok_hip.h: latok_pretokens_utf8_bytes_batch, latok_bpe_create_pretok), the parts that need no device:
the entry points exist in the library, the header and latok_amd/_lib.py with one arity and the header stays C99; pretok.h, compiled by
g++ (once more with the address and undefined-behaviour sanitizers, as a stand-alone program), cuts strings by its scalar walk AND word
by word as the device kernel does, exactly as tests/helpers/pretok_ref.py -- a plain restatement of the definition over bytes -- does:
the worked table, random text, malformed bytes; the reference itself is held to the ``regex`` package where that is installed; the
class ranges of tests/golden/pretok_classes.json are held to ``regex`` and to ``unicodedata``; the GPT-2 file loader gives the rank
order, the ids and the special tokens of the recorded vocabulary; the calls refuse bad arguments before they ask for a device."""
import ctypes as C
import json
import os
import random
import re
import subprocess
import sys
import unicodedata

import pytest

from conftest import GOLDEN, ROOT
from helpers import bpe_ref
from helpers import pretok_ref as ref

ENTRIES = {"latok_pretokens_utf8_bytes_batch": 11, "latok_bpe_create_pretok": 9, "latok_bpe_pretokenizer": 2}
PATTERN = r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"
MALFORMED = [b"\x80", b"\xbf", b"\xc0\x80", b"\xc1\xbf", b"\xc2", b"\xe0\x80\x80", b"\xe0\xa0", b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xf0\x80\x80\x80",
             b"\xf0\x9f\xa4", b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xf8\x88\x80\x80\x80", b"\xfe", b"\xff", b"\xe3\x80\x80", b"\xe3\x80\x80\x80",
             b"\xf0\x9d\x9f\x98", b"\xf0\x9d\x9f\x98\x80", b"a", b"1", b" ", b"'", b"s", b"'ll", b"\xc2\xa0", b"\xc3\xa9", b"\n", b"a\x80", b" \x80",
             b"'\x80", b"'s\x80"]


def _header_decl(name):
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    m = re.search(r"^int %s\((.*?)\);" % name, text, re.S | re.M)
    assert m, "%s is not declared in include/latok_hip.h" % name
    args = re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " "))
    return [a.strip() for a in args.split(",")]


def worked():
    with open(os.path.join(GOLDEN, "pretok_worked.json"), encoding="utf-8") as f:
        return json.load(f)["cases"]


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
    assert "latok_debug_pretok_limits" in exported
    assert len(_header_decl("latok_bpe_info")) == 8 and len(_header_decl("latok_bpe_create")) == 8     # the existing calls keep their arity
    for name in ("pretokens_utf8_csr", "pretokenize_utf8_batch", "pretokenize_batch"):
        assert callable(getattr(batch, name)), name
    assert callable(batch.BPE.from_gpt2_files) and callable(batch.BPE.gpt2_word_list)
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    comment = text[:text.index("#define LATOK_PRETOK_LATOK")].rsplit("/*", 1)[1]
    for needle in (PATTERN, "CHARACTERS", "CLASSES", "White_Space", "25 code points", "001C-001F", "SCAN START", "CONTRACTION", "FORCED",
                   "Unicode 13.0.0", "latok_set_rules has no influence", "7 behind", "6 ahead", "max_bytes", "cl100k_base", "add_prefix_space",
                   "flow form", "DevicePool", "before any device work", "lead_space = 1"):
        assert needle in comment, needle
    assert "#define LATOK_PRETOK_LATOK 0" in text and "#define LATOK_PRETOK_GPT2 1" in text
    assert (_lib.PRETOK_LATOK, _lib.PRETOK_GPT2) == (0, 1)


def test_limits_hook():
    from latok_amd import _lib
    import numpy as np
    fn = _lib.load().latok_debug_pretok_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(4, np.int64)
    assert fn(out.ctypes.data, 4) == 4
    assert out[0] == 64 and out[1] == 64 * out[0] and out[2] % 64 == 0 and 0 < out[2] <= 1024 and 7 <= out[3] <= out[0]
    assert fn(out.ctypes.data, 2) == 2 and fn(None, 4) < 0


def test_header_with_the_new_calls_is_c99_and_the_example_compiles(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "latok_hip.h"\n'
                   "int f(const uint8_t* u, const int64_t* o, int64_t* cnt, int64_t* sp, int64_t* n) {\n"
                   "    latok_bpe* w = NULL;\n"
                   "    int pt = -1;\n"
                   "    int rc = latok_bpe_create_pretok(u, o, 1, NULL, 4096, 0, LATOK_PRETOK_GPT2, 7u, &w);\n"
                   "    rc += latok_bpe_pretokenizer(w, &pt);\n"
                   "    rc += latok_pretokens_utf8_bytes_batch(u, o, 1, -1, LATOK_PRETOK_GPT2, cnt, sp, 64, n, LATOK_OUT_INT32, NULL);\n"
                   "    rc += latok_pretokens_utf8_bytes_batch(u, o, 1, -1, LATOK_PRETOK_LATOK, cnt, sp, 64, n, 0, NULL);\n"
                   "    return rc + pt + latok_bpe_destroy(w);\n}\n")
    strict = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c"]
    subprocess.check_call(strict + [str(src), "-o", str(tmp_path / "use.o")])
    subprocess.check_call(strict + [os.path.join(ROOT, "examples", "bpe_gpt2_utf8.c"), "-o", str(tmp_path / "example.o")])


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_the_reference_gives_the_worked_table():
    cases = worked()
    assert len(cases) >= 200
    for c in cases:
        assert ref.starts(c["text"].encode()) == c["starts"], c["text"]
    # every byte lies in exactly one pre-token
    for c in cases:
        b = c["text"].encode()
        spans = ref.pretokens(b)
        assert b"".join(b[a:e] for a, e in spans) == b and all(e > a for a, e in spans)
    assert ref.pretokens(b"don't  stop\n") == [(0, 3), (3, 5), (5, 6), (6, 11), (11, 12)]
    assert ref.pretokens(b"it'") == [(0, 2), (2, 3)] and ref.starts(b"s") == [0]


def test_the_reference_agrees_with_the_regex_package():
    regex = pytest.importorskip("regex")
    pat = regex.compile(PATTERN)
    rng = random.Random(1)
    for _ in range(200000):
        t = ref.random_text(rng)
        at, pos = [], 0          # byte offset of every match start, without re-encoding the prefix each time
        enc = [len(ch.encode()) for ch in t]
        prefix = [0]
        for n in enc:
            prefix.append(prefix[-1] + n)
        at = [prefix[m.start()] for m in pat.finditer(t)]
        assert ref.starts(t.encode()) == at, t


def test_the_golden_classes_agree_with_the_regex_package():
    """every scalar value; only code points that are unassigned (Cn) in the tables' Unicode version may be left out, because the package
    knows a later Unicode"""
    regex = pytest.importorskip("regex")
    with open(ref.GOLDEN) as f:
        unassigned = json.load(f)["Cn"]
    pats = {"S": regex.compile(r"\s"), "L": regex.compile(r"\p{L}"), "N": regex.compile(r"\p{N}")}
    left_out, k = 0, 0
    for cp in range(0x110000):
        if 0xD800 <= cp <= 0xDFFF:
            continue
        while k < len(unassigned) and unassigned[k][1] < cp:
            k += 1
        if k < len(unassigned) and unassigned[k][0] <= cp:
            left_out += 1
            assert ref.cp_class(cp) == "O", hex(cp)
            continue
        ch = chr(cp)
        want = "S" if pats["S"].match(ch) else "L" if pats["L"].match(ch) else "N" if pats["N"].match(ch) else "O"
        assert ref.cp_class(cp) == want, hex(cp)
    assert left_out < 0x110000 * 0.9


def test_the_golden_classes_agree_with_unicodedata():
    t = ref.tables()
    if unicodedata.unidata_version != t["version"]:
        pytest.skip("unicodedata is Unicode %s, the tables are %s" % (unicodedata.unidata_version, t["version"]))
    spaces = 0
    for cp in range(0x110000):
        cat = unicodedata.category(chr(cp))[0]
        got = ref.cp_class(cp)
        if got == "S":
            spaces += 1
            continue
        assert got == ("L" if cat == "L" else "N" if cat == "N" else "O"), hex(cp)
    assert spaces == 25 and ref.cp_class(0x1C) == "O" and ref.cp_class(0x1F) == "O" and ref.cp_class(0x3000) == "S"


# ---- pretok.h on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    """the stand-alone program, built by plain g++ and once more with -fsanitize=address,undefined; it is run directly"""
    exe = tmp_path_factory.mktemp("pretok_" + request.param) / "pretok_harness"
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "pretok_harness.cpp"), "-o", str(exe)])

    def run(script):
        out = subprocess.run([str(exe)], input=script, capture_output=True, text=True)
        assert out.returncode == 0, ({3: "the word form and the scalar walk disagree"}.get(out.returncode, out.returncode), out.stderr[-2000:])
        return out.stdout.splitlines()

    return run


def _check(harness, batches):
    """every string of every batch (a batch is packed as the device gets it: the strings share words and windows) against the reference"""
    lines = []
    for b in batches:
        lines.append("B %d" % len(b))
        lines += [s.hex() or "-" for s in b]
    got = harness("\n".join(lines) + "\n")
    assert len(got) == sum(len(b) for b in batches)
    k = 0
    for b in batches:
        for s in b:
            g = [] if got[k] == "-" else [int(x) for x in got[k].split()]
            assert g == ref.starts(s), (s, g, ref.starts(s))
            k += 1


def test_the_worked_table(harness):
    blobs = [c["text"].encode() for c in worked()]
    _check(harness, [[b] for b in blobs] + [blobs, blobs[::-1], [b"", b""] + blobs[:40] + [b""]])


def test_random_text(harness):
    rng = random.Random(5)
    batches, n = [], 0
    while n < 20000:
        batches.append([ref.random_text(rng, 40).encode() for _ in range(rng.randint(1, 40))])
        n += len(batches[-1])
    _check(harness, batches)


def test_malformed_bytes(harness):
    rng = random.Random(6)
    # a lead byte as a string's last byte followed by a string that starts with a continuation byte, and the like
    fixed = [[b"a\xe3", b"\x80\x80b"], [b"\xf0\x9f", b"\xa4\x93"], [b"it'", b"s"], [b"it'l", b"l"], [b" ", b"a"], [b"\xe3\x80", b"\x80"], [b"\xc2"], [b"\x80"],
             [b"\xff" * 70], [b"\x80" * 130], [b"\xe3" + b"\x80" * 66 + b"a"]]
    _check(harness, fixed)
    _check(harness, [[b"".join(rng.choice(MALFORMED) for _ in range(rng.randint(0, 12))) for _ in range(rng.randint(1, 40))] for _ in range(400)])
    _check(harness, [[bytes(rng.randrange(256) for _ in range(rng.randint(0, 200))) for _ in range(10)] for _ in range(150)])


def test_every_feature_at_every_offset_across_a_word_edge(harness):
    """the word form computes a word from a window: every feature of the rule is moved byte by byte across the edge of two words, with a
    string end on either side of it"""
    features = [b"a's b", b"we'll go", b"x 's", b"!'s", b"a \nb", b"a  b", b"a\xc2\xa0\xc2\xa0b", b"a\xe3\x80\x80\xe3\x80\x80b", b"a\xe3\x80\x80 b", b" a", b" 1",
                b" !", b"\xf0\x9d\x9f\x98\xf0\x9f\xa4\x93", b"\xf0\x9d\x9f\x98\xf0\x90\x80\x80", b"a\xe3\x80\x80's"]
    batches = []
    for f in features:
        for pad in range(64 - len(f) - 2, 66):
            batches.append([b"x" * pad + f])
            for cut in range(1, len(f)):
                batches.append([b"y" * pad + f[:cut], f[cut:] + b" z"])
    _check(harness, batches)


def test_the_class_function_gives_the_golden_classes(harness):
    names = "OLNS"
    cps = list(range(0, 0x3100)) + list(range(0xD7F0, 0xE010)) + list(range(0xFF00, 0x10400, 7)) + list(range(0x1D400, 0x1D800)) + [0x10FFFF, 0x1F913, 0x2FA1D]
    got = harness("".join("C %x\n" % cp for cp in cps))
    assert [names[int(g)] for g in got] == [ref.cp_class(cp) for cp in cps]


# ---- the GPT-2 file loader ---------------------------------------------------------------------------------------------------
def test_from_gpt2_files_gives_the_rank_order_the_ids_and_the_specials(tmp_path, monkeypatch):
    from latok_amd import batch
    model = os.path.join(GOLDEN, "pretok_gpt2")
    vocab_json, merges_txt = os.path.join(model, "vocab.json"), os.path.join(model, "merges.txt")
    words, ids, specials = batch.BPE.gpt2_word_list(vocab_json, merges_txt)
    vocab = json.load(open(vocab_json, encoding="utf-8"))
    assert words[:256] == [bytes([b]) for b in range(256)] and len(words) == len(vocab) - 1 and specials == {"<|endoftext|>": 0}
    dec = batch.BPE.gpt2_byte_decoder()
    assert len(dec) == 256 and sorted(dec.values()) == list(range(256)) and dec["Ġ"] == 0x20 and dec["Ċ"] == 0x0A and dec["!"] == 0x21
    merges = [l.split(" ") for l in open(merges_txt, encoding="utf-8").read().split("\n")[1:] if l]
    assert [bytes(dec[c] for c in a + b) for a, b in merges] == words[256:]
    assert ids == [vocab["".join({v: k for k, v in dec.items()}[x] for x in w)] for w in words]
    # the recorded ids, by the two references over this word list (what the device call is held to on the GPU)
    d = bpe_ref.rank_dict(words)
    cases = json.load(open(os.path.join(GOLDEN, "pretok_gpt2_cases.json"), encoding="utf-8"))["cases"]
    assert len(cases) >= 200
    for c in cases:
        blob = c["text"].encode()
        got = [pid for a, e in ref.pretokens(blob) for pid, _, _ in bpe_ref.cut(blob[a:e], d, 4096, -1, ids)]
        assert got == c["ids"], c["text"]
    # the constructor gets the list, the ids and the pre-tokenizer; the specials land on the object
    made = []
    monkeypatch.setattr(batch.BPE, "__init__", lambda self, w, **kw: made.append((list(w), kw)))
    obj = batch.BPE.from_gpt2_files(vocab_json, merges_txt, max_bytes=99)
    assert made == [(words, dict(ids=ids, pretokenizer="gpt2", max_bytes=99))] and obj.specials == specials
    batch.BPE.from_gpt2_files(vocab_json, merges_txt, pretokenizer="latok", lead_space=True)
    assert made[1][1] == dict(ids=ids, pretokenizer="latok", lead_space=True)
    # a merge result that vocab.json lacks, a line that is no pair, a token outside the byte alphabet
    short = dict(vocab)
    gone = "".join(merges[5])
    del short[gone]
    (tmp_path / "vocab.json").write_text(json.dumps(short), encoding="utf-8")
    with pytest.raises(ValueError, match="not in vocab.json"):
        batch.BPE.gpt2_word_list(str(tmp_path / "vocab.json"), merges_txt)
    for bad in ("#version: 0.2\ne r\nhe\n", "e  r\n", "e r x\n"):
        (tmp_path / "merges.txt").write_text(bad, encoding="utf-8")
        with pytest.raises(ValueError, match="left right"):
            batch.BPE.gpt2_word_list(vocab_json, str(tmp_path / "merges.txt"))
    (tmp_path / "vocab.json").write_text(json.dumps({"a": 0, "b": 1, "a b": 2, "€x": 3, "<s>": 4}), encoding="utf-8")
    (tmp_path / "merges.txt").write_text("€ x\n", encoding="utf-8")
    with pytest.raises(ValueError, match="byte alphabet"):
        batch.BPE.gpt2_word_list(str(tmp_path / "vocab.json"), str(tmp_path / "merges.txt"))
    (tmp_path / "merges.txt").write_text("", encoding="utf-8")
    w, i, s = batch.BPE.gpt2_word_list(str(tmp_path / "vocab.json"), str(tmp_path / "merges.txt"))
    assert (w, i, s) == ([b"a", b"b"], [0, 1], {"a b": 2, "€x": 3, "<s>": 4})
    assert len(made) == 2


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_the_calls_refuse_bad_arguments_before_they_ask_for_a_device():
    code = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import _lib
lib = _lib.load()
words = np.frombuffer(b"abcde", np.uint8)
off = np.array([0, 2, 5], np.int64)
h = C.c_void_p()
def create(ls=0, pt=1, mb=4096, out=h):
    return lib.latok_bpe_create_pretok(words.ctypes.data, off.ctypes.data, 2, None, mb, ls, pt, 0, C.byref(out) if out is not None else None)
for kw, needle in ((dict(pt=2), "pretok"), (dict(pt=-1), "pretok"), (dict(pt=1, ls=1), "lead_space"), (dict(ls=2), "lead_space"), (dict(mb=0), "max_bytes"),
                   (dict(out=None), "bpe_out")):
    rc = create(**kw)
    assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), (kw, rc, _lib.last_error())
    assert not h.value
assert create() == _lib.ERR_NOT_INIT and create(pt=0, ls=1) == _lib.ERR_NOT_INIT and not h.value
pt = C.c_int(5)
assert lib.latok_bpe_pretokenizer(None, C.byref(pt)) == _lib.ERR_INVALID and pt.value == 5
u8, boff = np.frombuffer(b"abc def", np.uint8), np.array([0, 7], np.int64)
cnt, sp, n = np.full(2, -7, np.int64), np.full(16, -7, np.int64), C.c_int64(-3)
def spans(pretok, flags=0, n_out=n, cap=8):
    return lib.latok_pretokens_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, pretok, cnt.ctypes.data, sp.ctypes.data, cap,
                                                C.byref(n_out) if n_out is not None else None, flags, None)
for pretok in (2, -1, 1 << 20):
    assert spans(pretok) == _lib.ERR_INVALID and "pretok" in _lib.last_error()
for pretok in (0, 1):
    for flags in (4, 64, 1 << 20):
        assert spans(pretok, flags) == _lib.ERR_INVALID and "flag" in _lib.last_error(), (pretok, flags)
    assert spans(pretok) == _lib.ERR_NOT_INIT, pretok       # the missing device comes next, as for the spans call
assert lib.latok_token_spans_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, cnt.ctypes.data, sp.ctypes.data, 8, C.byref(n), 0, None) == _lib.ERR_NOT_INIT
assert (cnt == -7).all() and (sp == -7).all() and n.value == -3
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_the_python_wrappers_refuse_bad_arguments_before_any_device():
    """LATOK_DEVICE names a device no machine has: anything that reached the library's init would raise RuntimeError instead"""
    code = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import batch
for kw in (dict(pretokenizer="gpt-2"), dict(pretokenizer=1), dict(pretokenizer=None), dict(pretokenizer="gpt2", lead_space=True)):
    try:
        batch.BPE([b"a", "b"], **kw)
        raise SystemExit("no ValueError for %%r" %% (kw,))
    except ValueError:
        pass
u8, off = batch.pack_utf8([b"a b"])
for call in (lambda: batch.pretokens_utf8_csr(u8, off, "regex"), lambda: batch.pretokens_utf8_csr(u8, off, dtype=np.int16),
             lambda: batch.pretokenize_utf8_batch([b"a"], pretokenizer=0), lambda: batch.pretokenize_batch(["a"], "GPT2")):
    try:
        call()
        raise SystemExit("no ValueError")
    except ValueError:
        pass
assert batch.pretokenize_utf8_batch([]) == [] and batch.pretokenize_batch([]) == []
for kw in (dict(pretokenizer="gpt2"), dict(pretokenizer="latok", lead_space=True)):
    try:
        batch.BPE([b"a", "b"], **kw)
        raise SystemExit("no RuntimeError")
    except RuntimeError:
        pass
try:
    batch.pretokenize_utf8_batch([b"a b"])
    raise SystemExit("no RuntimeError")
except RuntimeError:
    pass
print("ok")
""" % ROOT
    env = dict(os.environ, LATOK_DEVICE="4095")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)
