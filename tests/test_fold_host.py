"""Case folding and accent stripping (include/latok_hip.h: latok_fold_utf8_bytes_batch), the parts that need no device: the entry
point exists in the library, the header and latok_amd/_lib.py with one arity, and its constants agree everywhere; the fixture
tests/golden/fold_map.json equals a fresh sweep of the interpreter's own data where the UCD versions match; tests/helpers/fold_ref.py
-- the definition restated over bytes -- equals the text-level expression of BERT's normalizer; fold_map.h, compiled by g++ (once
more with the address and undefined-behaviour sanitizers, as a stand-alone program), gives fold_ref's image for every code point
and fold_ref's bytes for malformed strings at every alignment inside a poisoned buffer; fold_ref is held to the `tokenizers`
package where that is installed; bad arguments are refused before a device is asked for."""
import ctypes as C
import importlib.util
import os
import random
import re
import struct
import subprocess
import sys
import unicodedata as ud

import numpy as np
import pytest

from helpers import fold_ref as ref
from helpers import utf8_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "latok_fold_utf8_bytes_batch"
# (the malformed strings of tests/test_gpu_join_tokens.py, and forms that decode to values no text holds)
SOFT = [b"ab\xe6\x97 cd", b"\xc3 x", b"lone \xf0\x9f\x98", b"end\xe6", b"next starts ascii", b"\xe6\x97\xa5\xe6", b"\xf0", b"x\xc3"]
HARD = [b"a\x80\x80\x80\x80b", b"\xa9 starts with a continuation byte"]
ODD = [b"\xff", b"\xfe\xff", b"\xf8\x88\x80\x80\x80", b"\xc0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xe0\x80\x80"]


def _header_text():
    return open(os.path.join(ROOT, "include", "latok_hip.h")).read()


# ---- the surface -----------------------------------------------------------------------------------------------------------
def test_entry_point_is_exported_declared_and_bound():
    from latok_amd import _lib, batch
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "latok_amd", "liblatok_hip.so")], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAME in exported and "latok_debug_fold_limits" in exported
    m = re.search(r"^int %s\((.*?)\);" % NAME, _header_text(), re.S | re.M)
    assert m, "%s is not declared in include/latok_hip.h" % NAME
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    res, bound = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(bound) == len(args) == 11, (len(bound), len(args))
    assert getattr(lib, NAME).argtypes == bound
    for a, b in zip(args, bound):
        if "*" in a:
            assert b is C.c_void_p or issubclass(b, C._Pointer), (a, b)
        else:
            assert b is (C.c_int64 if a.startswith("int64_t") else C.c_int), (a, b)
    for name in ("fold_utf8_csr", "fold_utf8_batch", "fold_batch"):
        assert callable(getattr(batch, name)), name


def test_constants_agree_between_header_binding_and_batch():
    from latok_amd import _lib, batch
    text = _header_text()
    want = {"LOWER": 1, "STRIP_MARKS": 2, "CLEAN": 4, "CJK_SPACE": 8}
    for key, val in want.items():
        m = re.search(r"^#define LATOK_FOLD_%s (\d+)$" % key, text, re.M)
        assert m and int(m.group(1)) == val, key
        assert getattr(_lib, "FOLD_" + key) == val and getattr(batch, "FOLD_" + key) == val and getattr(ref, key) == val
    assert batch.FOLD_UNCASED == 3 == ref.UNCASED
    inc = open(os.path.join(ROOT, "latok_amd", "csrc", "fold_tables.inc")).readline()
    assert inc.startswith("// unidata_version ") and inc.split()[2] == ref.UNIDATA_VERSION


def test_the_chained_calls_take_a_fold_keyword_that_defaults_to_off():
    import inspect
    from latok_amd import batch
    for name in ("wordpiece_ids_utf8_batch", "wordpiece_ids_batch", "wordpiece_encode_utf8_batch", "token_ids_utf8_batch",
                 "term_counts_utf8_batch", "hashed_term_counts_utf8_batch"):
        p = inspect.signature(getattr(batch, name)).parameters
        assert "fold" in p and p["fold"].default == 0, name
    for name in ("fold_utf8_csr", "fold_utf8_batch", "fold_batch"):
        assert inspect.signature(getattr(batch, name)).parameters["fold"].default == batch.FOLD_UNCASED


def test_limits_hook():
    from latok_amd import _lib
    fn = _lib.load().latok_debug_fold_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(3, np.int64)
    assert fn(out.ctypes.data, 3) == 3
    assert out[0] > 0 and out[0] % 16 == 0 and out[1] == 16 and out[2] == 3


def test_header_with_the_new_call_is_c99_and_the_example_compiles(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "latok_hip.h"\n'
                   "int f(const uint8_t* u, const int64_t* o, uint8_t* out, int64_t* off, int64_t* n) {\n"
                   "    return latok_fold_utf8_bytes_batch(u, o, 1, -1, LATOK_FOLD_LOWER | LATOK_FOLD_STRIP_MARKS | LATOK_FOLD_CLEAN | LATOK_FOLD_CJK_SPACE,\n"
                   "                                       out, 64, off, n, LATOK_DEVICE_PTRS, NULL);\n}\n")
    strict = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c"]
    subprocess.check_call(strict + [str(src), "-o", str(tmp_path / "use.o")])
    subprocess.check_call(strict + [os.path.join(ROOT, "examples", "fold_wordpiece_utf8.c"), "-o", str(tmp_path / "example.o")])


def test_the_comments_point_to_the_fold_call():
    text = _header_text()
    comment = text[:text.index("typedef struct latok_wordpiece")].rsplit("/*", 1)[1]
    for needle in (NAME, "BasicTokenizer", "final-sigma", "BPE", "flow form", "sentence pairs"):
        assert needle in comment, needle
    fold_comment = text[:text.index("#define LATOK_FOLD_LOWER")].rsplit("/*", 1)[1]
    for needle in ("CLEAN", "STRIP_MARKS", "CJK_SPACE", "U+0130", "U+03A3", "Hangul", "verbatim", "3 * total_bytes", "same string", "fold == 0",
                   "LATOK_ERR_INVALID", "latok_set_rules"):
        assert needle in fold_comment, needle
    from latok_amd import batch
    for needle in ("fold=FOLD_UNCASED", "BasicTokenizer", "final-sigma", "BPE", "flow form", "sentence pairs"):
        assert needle in batch.WordPiece.__doc__, needle
    assert "FOLDED" in batch.wordpiece_ids_utf8_batch.__doc__


def test_bad_arguments_are_refused_before_any_device():
    code = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import _lib, batch
lib = _lib.load()
u8, boff = np.frombuffer(b"Abc D\xc3\x89f", np.uint8), np.array([0, 8], np.int64)
out, off, n = np.full(32, 0x5A, np.uint8), np.full(2, -7, np.int64), C.c_int64(0)
def call(fold=3, flags=0, o=out, cap=24, of=off, pn=n):
    return lib.latok_fold_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 8, fold, o.ctypes.data if o is not None else None, cap,
                                           of.ctypes.data if of is not None else None, C.byref(pn) if pn is not None else None, flags, None)
for fold in (16, 32, -1, 1 << 20, 15 | 64):
    assert call(fold=fold) == _lib.ERR_INVALID and "fold" in _lib.last_error(), fold
for flags in (2, 4, 64, 1 << 20):
    assert call(flags=flags) == _lib.ERR_INVALID and "flag" in _lib.last_error(), flags
assert call(of=None) == _lib.ERR_INVALID and "out_off" in _lib.last_error()
assert call(o=None) == _lib.ERR_INVALID and "out_bytes" in _lib.last_error()
assert call(cap=-1) == _lib.ERR_INVALID and "capacity" in _lib.last_error()
assert call(pn=None) == _lib.ERR_INVALID
assert call() == _lib.ERR_NOT_INIT
assert (out == 0x5A).all() and (off == -7).all()
for bad in (16, -1, 1.0, True, "lower", None):
    for f in (lambda: batch.fold_utf8_batch([b"a"], bad), lambda: batch.fold_batch(["a"], bad), lambda: batch.fold_utf8_csr(u8, boff, bad)):
        try:
            f()
        except ValueError as e:
            assert "fold" in str(e), e
        else:
            raise AssertionError(bad)
assert batch.fold_utf8_batch([]) == [] and batch.fold_batch([]) == []
print("ok")
""" % ROOT
    env = dict(os.environ, LATOK_DEVICE="4095")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


# ---- the fixture and the reference against the live interpreter ---------------------------------------------------------------
def _load_generator():
    spec = importlib.util.spec_from_file_location("make_fold_golden", os.path.join(ROOT, "tests", "golden", "make_fold_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_equals_a_fresh_sweep_of_the_interpreter():
    if ud.unidata_version != ref.UNIDATA_VERSION:
        pytest.skip("this interpreter carries UCD %s, the fixture was written from UCD %s" % (ud.unidata_version, ref.UNIDATA_VERSION))
    import json
    fresh = _load_generator().sweep()
    assert fresh == json.load(open(os.path.join(ROOT, "tests", "golden", "fold_map.json")))
    # the statistics of the definition
    rows = fresh["map"]
    assert sum(lo != [c] for c, lo, _ in rows) == 1393
    assert sum(st != [c] for c, _, st in rows) == 3882 and len(rows) == 4895


def test_fixture_bounds_the_image_and_the_growth():
    """the size rule out_off[n_str] <= 3 * total_bytes, derived from the fixture: the largest image and the largest growth over every
    code point and every flag combination"""
    max_cps = max_bytes = 0
    growth = 0.0
    some = set(ref.LOWER_OF) | {ref.S_BASE, ref.S_BASE + 1, ref.S_BASE + ref.S_COUNT - 1} | set(ref.ZS) | {0x4E00, 0x3400, 0x20000, 0xF900, 0x2F800}
    some |= set(range(0x80)) | {0x7FF, 0x800, 0xFFFF, 0x10000}
    for fold in range(16):
        for c in some:
            img = ref.fold_cp(c, fold)
            src = len(ref.encode([c]))
            max_cps, max_bytes = max(max_cps, len(img)), max(max_bytes, len(ref.encode(img)))
            growth = max(growth, len(ref.encode(img)) / src)
    # every Hangul syllable: 3 bytes in, 2 or 3 jamo of 3 bytes out; every CJK ideograph: itself between two spaces
    for s in range(ref.S_COUNT):
        img = ref.fold_cp(ref.S_BASE + s, ref.ALL)
        assert len(img) in (2, 3) and all(0x1100 <= x <= 0x11FF for x in img)
    for a, b in ref.CJK_RANGES:
        for c in (a, b):
            assert len(ref.encode(ref.fold_cp(c, ref.ALL))) <= 2 + 4 and len(ref.encode([c])) >= 3
    assert max_cps == 3 and max_bytes == 12 and growth == 3.0
    assert ref.fold_cp(0x1D160, ref.STRIP_MARKS) == [0x1D158, 0x1D165, 0x1D16E] and ref.fold_cp(0x0130, ref.LOWER) == [0x69, 0x307]
    assert ref.fold_cp(0x03A3, ref.LOWER) == [0x03C3] and ref.fold_cp(0x0301, ref.STRIP_MARKS) == []


def _bert_text(t):
    return "".join(ch for ch in ud.normalize("NFD", t.lower()) if ud.category(ch) != "Mn")


def test_reference_equals_the_text_level_expression_of_bert():
    if ud.unidata_version != ref.UNIDATA_VERSION:
        pytest.skip("this interpreter carries UCD %s, the fixture was written from UCD %s" % (ud.unidata_version, ref.UNIDATA_VERSION))
    reorder = [c for c in range(0x110000) if ud.combining(chr(c)) != 0 and ud.category(chr(c)) != "Mn"]
    assert len(reorder) == 23
    avoid = set(reorder) | {0x03A3} | set(range(0xD800, 0xE000))
    rng = random.Random(11)
    pool = [c for c in list(ref.LOWER_OF) + list(range(0x20, 0x3000)) + list(range(0xAC00, 0xAC80)) + [0x4E00, 0x1F600, 0x1D160] if c not in avoid]
    for _ in range(3000):
        t = "".join(chr(rng.choice(pool)) for _ in range(rng.randint(0, 12)))
        assert ref.fold_bytes(t.encode(), ref.UNCASED).decode() == _bert_text(t), [hex(ord(c)) for c in t]
    # and what is out of scope does differ: the final sigma
    assert ref.fold_bytes("ΟΔΟΣ".encode(), ref.UNCASED).decode() == "οδοσ" != _bert_text("ΟΔΟΣ")


def test_reference_follows_the_byte_rule():
    U = ref.UNCASED
    assert ref.fold_blobs([b"x\xc3", b"\xa9y"], U) == [b"x\xc3", b"\xa9y"] and ref.fold_bytes(b"x\xc3\x89y", U) == b"xey"
    assert ref.fold_bytes(b"\xc1\x81", ref.LOWER) == b"a" and ref.fold_bytes(b"\xc1\x81", 0) == b"\xc1\x81"
    assert ref.fold_bytes(b"\xc1\x81", ref.STRIP_MARKS) == b"\xc1\x81"                    # an overlong form survives where its image is itself
    assert ref.fold_bytes(b"\xef\xbf\xbd\x80\x00\x7f\tA", ref.CLEAN) == b"\x80 A"           # U+FFFD, NUL, DEL dropped; the stray byte stays
    assert ref.fold_bytes("日A".encode(), ref.CJK_SPACE) == " 日 A".encode()
    for blob in SOFT + HARD + ODD:                     # verbatim apart from the ASCII letters (U+65E5 and U+8000 are their own image)
        assert ref.fold_bytes(blob, U) == bytes(b + 32 if 0x41 <= b <= 0x5A else b for b in blob), blob
    for fold in ref.COMBOS:
        u8, off = cases.string_start_case()
        a, b = ref.fold_batch(u8, off, fold), ref.fold_batch_scalar(u8, off, fold)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), fold


# ---- fold_map.h on the host ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    """the stand-alone program, built by plain g++ and once more with -fsanitize=address,undefined; it is run directly"""
    d = tmp_path_factory.mktemp("fold_" + request.param)
    exe = d / "fold_harness"
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "fold_harness.cpp"), "-o", str(exe)])

    def run(*args):
        out = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr[-2000:])

    run.dir = d
    return run


@pytest.mark.parametrize("fold", [ref.LOWER, ref.STRIP_MARKS, ref.CLEAN, ref.CJK_SPACE, ref.UNCASED, ref.ALL])
def test_fold_map_h_gives_the_reference_image_of_every_code_point(harness, fold):
    path = harness.dir / ("sweep_%d.bin" % fold)
    harness("sweep", fold, path)
    got = np.fromfile(str(path), np.uint32).reshape(ref.N_CP + 1, 4)
    n, cps = ref.dense(fold)
    bad = np.flatnonzero((got[:, 0] != n) | (got[:, 1:] != cps).any(axis=1))
    assert bad.size == 0, [(hex(c), got[c].tolist(), n[c], cps[c].tolist()) for c in bad[:8]]
    # (the dense table is the reference itself on every code point it lists, and the identity elsewhere: spot-check the latter)
    rng = random.Random(fold)
    for c in [rng.randrange(ref.N_CP) for _ in range(2000)]:
        img = ref.fold_cp(c, fold)
        assert n[c] == len(img) and cps[c, :len(img)].tolist() == img, hex(c)


def _byte_cases():
    rng = random.Random(5)
    blobs = list(cases.sequences()) + SOFT + HARD + ODD + [b"", b"A", b"x\xc3", b"\xa9y", b"x\xc3\x89y", b"\xc1\x81"]
    blobs += [bytes(w) + b"a" for w in cases.windows(0xC0)[::97].tolist()]
    blobs += [data for data, _ in cases.end_of_batch_cases()[::41]]
    alphabet = ["É", "Ⱥ", "K", "각", "𝅘𝅥𝅮", "́", "日", "A", " ", "\t", "\x00", "­", "　", "ß", "İ", "z"]
    for _ in range(300):
        t = "".join(rng.choice(alphabet) for _ in range(rng.randint(1, 24))).encode()
        cut = rng.randint(0, 3)
        blobs.append(t[:len(t) - cut] if rng.random() < 0.5 else t)
    return blobs


def test_fold_map_h_folds_byte_strings_as_the_reference_at_every_alignment(harness):
    blobs = _byte_cases()
    work = [(fold, b) for fold in ref.COMBOS for b in blobs]
    src, dst = harness.dir / "cases.bin", harness.dir / "cases.out"
    with open(src, "wb") as f:
        for fold, b in work:
            f.write(struct.pack("<ii", fold, len(b)) + b)
    harness("bytes", src, dst)
    data, p = open(dst, "rb").read(), 0
    for fold, b in work:
        (n,) = struct.unpack_from("<i", data, p)
        got = data[p + 4:p + 4 + n]
        p += 4 + n
        assert got == ref.fold_bytes(b, fold), (fold, b, got)
    assert p == len(data)


# ---- the reference against the tokenizers package ----------------------------------------------------------------------------
TK_WORDS = ["Café", "RÉSUMÉ", "naïve", "Ångström", "Übergröße", "Straße", "Tiếng", "Việt", "NGUYỄN", "Đường", "phở", "Ελληνικά", "ΑΘΗΝΑ", "Άλφα",
            "Привет", "МОСКВА", "ёлка", "Й", "हिन्दी", "नमस्ते", "क़िला", "한국어", "각", "서울", "İstanbul", "ǅ", "ﬁn", "plain", "MiXeD", "x"]


def test_reference_agrees_with_the_tokenizers_package_on_the_word_list():
    tk = pytest.importorskip("tokenizers")
    norm = tk.normalizers.BertNormalizer(clean_text=False, handle_chinese_chars=False, strip_accents=True, lowercase=True)
    assert not any("Σ" in w for w in TK_WORDS)
    for w in TK_WORDS:
        assert ref.fold_bytes(w.encode(), ref.UNCASED).decode() == norm.normalize_str(w), w
