"""Decoding (include/latok_hip.h: latok_detok_*), the parts that need no device: the entry points exist in the library, the header and
latok_amd/_lib.py with one arity and the header stays C99; the example compiles; the limits hook answers; detok.h, compiled by g++ (once
more with the address and undefined-behaviour sanitizers, as a stand-alone program), builds its object and decodes CSR batches exactly as
tests/helpers/detok_ref.py -- a plain restatement of the rule over Python lists and a dict -- does: both modes, dense and sorted maps on
either side of the threshold, extreme ids, duplicate ids, the empty word, the bare prefix, a word holding the separator, an empty prefix,
V = 0, rows that are empty / all skipped / all unknown, a row that begins with a continuation word, runs of dropped pieces at row starts
and across row edges, blob reads at every dword phase inside a poisoned buffer; the look-back bound is counted; the reference itself is
held to sep.join(..).replace(..) and, where installed, to the `tiktoken` package; latok_detok_create and the calls refuse bad arguments
before they ask for a device."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import pytest

from helpers import detok_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"latok_detok_create": 9, "latok_detok_destroy": 1, "latok_detok_info": 8, "latok_detok_csr": 14, "latok_detok_padded": 14}
SEEDS = (1, 2, 3)


def _limits():
    import numpy as np
    from latok_amd import _lib
    fn = _lib.load().latok_debug_detok_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(5, np.int64)
    assert fn(out.ctypes.data, 5) == 5
    return [int(x) for x in out]


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
            if "*" in a:
                assert b is C.c_void_p or issubclass(b, C._Pointer), (name, a, b)
            else:
                assert b is (C.c_int64 if a.startswith("int64_t") else C.c_int), (name, a, b)
    assert "latok_debug_detok_limits" in exported
    for name in ("Detokenizer", "decode_csr", "decode_padded", "decode_batch"):
        assert callable(getattr(batch, name)), name
    assert callable(batch.Detokenizer.from_tiktoken_file) and callable(batch.Detokenizer.from_vocab_file)
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    comment = text[text.index("/* Decoding:"):text.index("typedef struct latok_detok")]
    for needle in ("LOWEST INDEX", "empty word", "CONTINUATION", "dense", "bisection", "DROPPED", "unknown", "skip_ids", "HOST pointer",
                   "decode_bytes", '" ".join(tokens).replace(" ##", "")', "sep.join(words).replace(sep + prefix", "LATOK_OUT_INT32",
                   "latok_tfidf_csr", "latok_fold_utf8_bytes_batch", "size query", "LATOK_ERR_INVALID", "lengths == NULL", "16-byte aligned",
                   "flow form", "Unigram"):
        assert needle in comment, needle


def test_limits_hook():
    from latok_amd import _lib
    block, win, spread, chunk, lane = _limits()
    assert block > 0 and block % 64 == 0 and win >= 1024 and win % 16 == 0 and spread >= 1 and chunk > 0 and 0 < lane < win
    fn = _lib.load().latok_debug_detok_limits
    import numpy as np
    out = np.zeros(5, np.int64)
    assert fn(out.ctypes.data, 2) == 2 and fn(None, 4) < 0


def test_header_with_the_new_calls_is_c99_and_the_example_compiles(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "latok_hip.h"\n'
                   "int f(const uint8_t* u, const int64_t* o, const int32_t* ids, const int32_t* len, uint8_t* out, int64_t* off, int64_t* n) {\n"
                   "    latok_detok* d = NULL;\n"
                   "    int64_t a, b, c, e; int mode, dense, dev;\n"
                   "    int rc = latok_detok_create(u, o, 1, NULL, LATOK_DETOK_WORDPIECE, u, 2, 32, &d);\n"
                   "    rc += latok_detok_info(d, &a, &b, &c, &e, &mode, &dense, &dev);\n"
                   "    rc += latok_detok_csr(d, o, ids, 1, 4, ids, 2, out, 64, off, n, NULL, LATOK_DEVICE_PTRS | LATOK_OUT_INT32, NULL);\n"
                   "    rc += latok_detok_padded(d, ids, len, 1, 4, NULL, 0, NULL, 0, off, n, n, 0, NULL);\n"
                   "    return rc + latok_detok_destroy(d) + LATOK_DETOK_CONCAT;\n}\n")
    strict = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c"]
    subprocess.check_call(strict + [str(src), "-o", str(tmp_path / "use.o")])
    subprocess.check_call(strict + [os.path.join(ROOT, "examples", "detok_utf8.c"), "-o", str(tmp_path / "example.o")])


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_the_reference_gives_the_worked_cases():
    words = [b"[CLS]", b"un", b"##aff", b"##able", b"[SEP]", b"##", b"a b", b""]
    d = ref.id_map(words)
    assert ref.decode_row([0, 1, 2, 3, 4], d, ref.WORDPIECE, skip=(0, 4)) == (b"unaffable", 0)
    assert ref.decode_row([2, 3, 1], d, ref.WORDPIECE) == (b"##affable un", 0)            # w_0 verbatim, prefix included
    assert ref.decode_row([1, 5, 99, 1], d, ref.WORDPIECE) == (b"un ## un", 1)             # the bare prefix is no continuation word
    assert ref.decode_row([1, 7, 1], d, ref.WORDPIECE) == (b"un  un", 0)                   # the empty word still gets its separator
    assert ref.decode_row([1, 2, 3], d, ref.CONCAT) == (b"un##aff##able", 0)
    assert ref.decode_row([1, 2], d, ref.WORDPIECE, prefix=b"") == (b"un##aff", 0)         # an empty prefix: every word continues
    assert ref.decode([[], [99], [0]], d, skip=(0,)) == ([b"", b"", b""], 1)
    assert ref.id_map([b"a", b"b", b"c"], [5, 5, -1]) == {5: b"a", -1: b"c"}


@pytest.mark.parametrize("seed", SEEDS)
def test_the_reference_is_join_and_replace_where_the_vocabulary_allows_it(seed):
    rng = random.Random(seed)
    for prefix, sep in ((b"##", b" "), (b"@", b"_"), (b"\xc4\xa0", b"\n")):
        alphabet = [bytes([c]) for c in b"abcxyz\xc3\xa9"]
        words = set()
        while len(words) < 60:
            w = b"".join(rng.choice(alphabet) for _ in range(rng.randint(1, 5)))
            words.add(w if rng.random() < 0.5 else prefix + w)
        words = sorted(words)
        assert all(sep not in w and w != prefix for w in words)
        d = ref.id_map(words)
        for _ in range(200):
            row = [rng.randrange(len(words)) for _ in range(rng.randint(0, 9))]
            assert ref.decode_row(row, d, ref.WORDPIECE, prefix, sep)[0] == ref.join_replace([words[i] for i in row], prefix, sep), row


def test_the_reference_agrees_with_the_tiktoken_package():
    tiktoken = pytest.importorskip("tiktoken")
    words = [bytes([b]) for b in range(256)] + [b"ab", b"abc", b" the", b"\xc3\xa9"]
    enc = tiktoken.Encoding("worked", pat_str=r"[\s\S]+", mergeable_ranks={w: i for i, w in enumerate(words)}, special_tokens={})
    rng = random.Random(5)
    d = ref.id_map(words)
    for _ in range(300):
        row = [rng.randrange(len(words)) for _ in range(rng.randint(0, 12))]
        assert ref.decode_row(row, d)[0] == enc.decode_bytes(row), row


# ---- detok.h on the host -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    """the stand-alone program, built by plain g++ and once more with -fsanitize=address,undefined; it is run directly"""
    exe = tmp_path_factory.mktemp("detok_" + request.param) / "detok_harness"
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "detok_harness.cpp"), "-o", str(exe)])

    def run(script, poison=0xA5):
        out = subprocess.run([str(exe)], input="%02x\n" % poison + script, capture_output=True, text=True)
        assert out.returncode == 0, ({3: "a blob load left the blob", 4: "a map or entry load left its array",
                                      5: "the count pass and the write pass disagree"}.get(out.returncode, out.returncode), out.stderr[-2000:])
        return out.stdout.splitlines()

    return run


def _run(harness, words, batches, ids=None, mode=ref.CONCAT, prefix=b"", sep=0, wins=(4096, 1, 3, 7), poisons=(0x00, 0xFF, 0xA5)):
    """every batch (rows, skip) at every window size and poison, against the reference and the look-back bound; returns the info"""
    d = ref.id_map(words, ids)
    lines = ["V %d %s %d %d" % (mode, prefix.hex() or "-", sep, len(words))]
    lines += ["%s %s" % ("-" if ids is None else ids[i], w.hex() or "-") for i, w in enumerate(words)]
    cases = [(win, rows, skip) for rows, skip in batches for win in wins]
    for win, rows, skip in cases:
        lines.append("D %d %d %s %d %s" % (win, len(skip), " ".join(map(str, skip)), len(rows),
                                           " ".join("%d %s" % (len(r), " ".join(map(str, r))) for r in rows)))
    info = None
    for poison in poisons:      # what pads a word in the blob must not reach the output
        out = harness("\n".join(lines) + "\n", poison)
        m = re.match(r"words (\d+) ids (\d+) dense (\d) max (\d+) blob (\d+)$", out[0])
        assert m, out[:2]
        info = dict(zip(("n_words", "n_ids", "dense", "max_len", "blob_bytes"), map(int, m.groups())))
        assert info["n_words"] == len(words) and info["n_ids"] == len(d) and info["max_len"] == max([len(w) for w in words] + [0])
        assert info["blob_bytes"] == sum((len(w) + 3) // 4 * 4 for w in words)
        at = 1
        for win, rows, skip in cases:
            want, unknown = ref.decode(rows, d, mode, prefix, bytes([sep]), skip)
            m = re.match(r"unknown (\d+) walks (\d+) bytes (\d+)$", out[at])
            assert m, out[at]
            n_pieces = sum(len(r) for r in rows)
            assert int(m.group(1)) == unknown and int(m.group(3)) == sum(map(len, want)), (rows, skip, out[at])
            assert int(m.group(2)) <= n_pieces, ("the walks of a batch total at most its piece count", rows, out[at])
            if mode == ref.CONCAT:
                assert int(m.group(2)) == 0
            got = [bytes.fromhex(x) if x != "-" else b"" for x in out[at + 1:at + 1 + len(rows)]]
            assert got == want, (poison, win, rows, skip, got, want)
            at += 1 + len(rows)
        assert at == len(out)
    return info


WP_WORDS = [b"[PAD]", b"[CLS]", b"[SEP]", b"un", b"##aff", b"##able", b"##", b"a b", b"", b"##\xc3\xa9t\xc3\xa9", b"x", b"##y", b"#", b"###"]


def test_both_modes_on_a_worked_vocabulary(harness):
    rows = [[1, 3, 4, 5, 2, 0, 0], [], [4, 5, 3], [3, 6, 3], [3, 8, 3], [8], [8, 8], [3, 7, 11], [9, 9, 10, 12, 13], [0, 0, 0], [77, -5], [1, 77, 3, 77, 0, 4],
            [1, 0, 2], [1], [3]]
    batches = [(rows, ()), (rows, (0, 1, 2)), (rows, (3,)), ([[]] * 5, ()), ([], ()), (rows, tuple(range(16)))]
    for mode, prefix, sep in ((ref.WORDPIECE, b"##", 0x20), (ref.WORDPIECE, b"", 0x5F), (ref.WORDPIECE, b"#", 0), (ref.WORDPIECE, b"[", 0xFF),
                              (ref.CONCAT, b"", 0)):
        info = _run(harness, WP_WORDS, batches, mode=mode, prefix=prefix, sep=sep)
        assert info["dense"] == 1 and info["n_ids"] == len(WP_WORDS)


def test_dropped_runs_in_front_of_a_kept_word_at_row_starts_and_across_row_edges(harness):
    skip = (0, 1, 2)
    rows = [[1, 3], [0, 0, 0, 3], [0] * 9 + [4, 3], [99] * 5 + [3, 99, 99, 4, 0, 3], [3] + [0] * 7, [0] * 8, [3, 99, 0, 99, 3], [4], [0, 4, 5],
            [3, 0, 0, 0, 0, 0, 5, 0, 0, 10], [2] * 20, [10]]
    info = _run(harness, WP_WORDS, [(rows, skip), (rows, ())], mode=ref.WORDPIECE, prefix=b"##", sep=0x20)
    assert info["dense"] == 1


def test_dense_and_sorted_maps_on_either_side_of_the_threshold(harness):
    spread = _limits()[2]
    words = [b"w%d" % i for i in range(10)]
    for top, dense in ((spread * 10 - 1, 1), (spread * 10, 0), (1 << 20, 0)):
        ids = list(range(9)) + [top]                       # the id range is top + 1
        assert ref.is_dense(words, ids, spread) == bool(dense)
        probes = [[0, 8, top, top - 1, top + 1, -1, 9, 5], [top] * 3, []]
        assert _run(harness, words, [(probes, ()), (probes, (top, 0))], ids=ids)["dense"] == dense
    extreme = [ref.I32_MIN, ref.I32_MAX, -1, 0, 7, ref.I32_MIN + 1, ref.I32_MAX - 1, 100, -100, 5]
    probes = [extreme + [1, -2, ref.I32_MIN + 2, ref.I32_MAX - 2], [ref.I32_MAX], [ref.I32_MIN]]
    assert _run(harness, words, [(probes, ()), (probes, (ref.I32_MIN, -1))], ids=extreme, mode=ref.WORDPIECE, prefix=b"w", sep=0x2C)["dense"] == 0
    near = [ref.I32_MAX - i for i in range(10)]            # a dense map that ends at INT32_MAX, and one that starts at INT32_MIN
    assert _run(harness, words, [([near + [ref.I32_MAX - 10, 0, ref.I32_MIN]], ())], ids=near)["dense"] == 1
    low = [ref.I32_MIN + 2 * i for i in range(10)]
    assert _run(harness, words, [([low + [ref.I32_MIN + 1, ref.I32_MIN + 19, ref.I32_MAX, -1]], ())], ids=low)["dense"] == 1


def test_duplicate_ids_duplicate_words_the_empty_word_and_an_empty_vocabulary(harness):
    words = [b"a", b"b", b"a", b"", b"c", b"b"]
    for ids in ([5, 5, 6, 7, 5, 8], [1000, -1000, 1000, 0, -1000, 1 << 30]):
        info = _run(harness, words, [([[5, 6, 7, 8, 1000, -1000, 0, 1 << 30], [7], []], ())], ids=ids)
        assert info["n_ids"] == len(set(ids))
    info = _run(harness, [], [([[0, 1, -1], [], [ref.I32_MIN]], ()), ([], ())])
    assert info["dense"] == 0 and info["n_ids"] == 0 and info["blob_bytes"] == 0
    _run(harness, [b""], [([[0, 0], [0]], ())], mode=ref.WORDPIECE, prefix=b"##", sep=0x20)


def test_blob_reads_at_every_dword_phase_and_every_stretch(harness):
    """prefixes of 0 .. 8 bytes put the continuation body at every phase; windows of 1 .. 9 bytes cut every word at every offset"""
    for plen in range(9):
        prefix = b"#@%&+=!?"[:plen]
        words = [prefix + bytes(range(65, 65 + n)) for n in range(1, 14)] + [bytes(range(97, 97 + n)) for n in range(1, 14)] + [prefix]
        rows = [list(range(len(words))), list(range(len(words) - 1, -1, -1)), [0, 13, 1, 14], [26, 26, 0]]
        _run(harness, words, [(rows, ())], mode=ref.WORDPIECE, prefix=prefix, sep=0x7C, wins=(1, 2, 3, 4, 5, 8, 9, 4096))
    long_words = [bytes((i * 7 + j) % 251 for j in range(n)) for i, n in enumerate((4095, 4096, 4097, 3 * 4096 + 5, 1, 0))]
    _run(harness, long_words, [([[0, 1, 2], [3, 4, 5, 4], [2, 2]], ())], wins=(4096, 64), poisons=(0xA5,))


@pytest.mark.parametrize("seed", SEEDS)
def test_random_vocabularies_and_batches(harness, seed):
    rng = random.Random(seed)
    spread = _limits()[2]
    for mode in (ref.CONCAT, ref.WORDPIECE):
        for n_words in (1, 7, 120):
            prefix = rng.choice((b"##", b"", b"\xc4\xa0")) if mode == ref.WORDPIECE else b""
            words = [(prefix if rng.random() < 0.4 else b"") + bytes(rng.choice(b"abc \xc3\xa9#") for _ in range(rng.randint(0, 9))) for _ in range(n_words)]
            ids = None if rng.random() < 0.3 else [rng.randrange(-50, 50 + (0 if rng.random() < 0.5 else spread * n_words * 3)) for _ in words]
            pool = (list(range(n_words)) if ids is None else ids) + [-1, 10 ** 6]
            rows = [[rng.choice(pool) for _ in range(rng.choice((0, 0, 1, 2, 5, 30)))] for _ in range(25)]
            skip = tuple(rng.sample(pool, min(len(pool), rng.randint(0, 4))))
            info = _run(harness, words, [(rows, ()), (rows, skip)], ids=ids, mode=mode, prefix=prefix, sep=rng.randrange(256) if mode else 0,
                        wins=(4096, 5), poisons=(0xA5,))
            assert info["dense"] == int(ref.is_dense(words, ids, spread))


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_create_and_the_calls_refuse_bad_arguments_before_they_ask_for_a_device():
    code = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import _lib
lib = _lib.load()
words = np.frombuffer(b"abcde", np.uint8)
pre = np.frombuffer(b"##______", np.uint8)
h = C.c_void_p()
def create(off, n, out=h, w=words, mode=1, plen=2, sep=32, p=pre):
    off = np.array(off, np.int64)
    return lib.latok_detok_create(w.ctypes.data if w is not None else None, off.ctypes.data, n, None, mode, p.ctypes.data if p is not None else None,
                                  plen, sep, C.byref(out) if out is not None else None)
for kw, needle in ((dict(off=[1, 2, 5], n=2), "start at 0"), (dict(off=[0, 3, 2], n=2), "non-decreasing"), (dict(off=[0, 2, 5], n=-1), "n_words"),
                   (dict(off=[0, 2, 5], n=1 << 31), "n_words"), (dict(off=[0, 1 << 32], n=1), "2^32"), (dict(off=[0, 2, 5], n=2, mode=2), "mode"),
                   (dict(off=[0, 2, 5], n=2, mode=-1), "mode"), (dict(off=[0, 2, 5], n=2, plen=9), "prefix_len"), (dict(off=[0, 2, 5], n=2, plen=-1), "prefix_len"),
                   (dict(off=[0, 2, 5], n=2, p=None), "prefix"), (dict(off=[0, 2, 5], n=2, sep=256), "sep"), (dict(off=[0, 2, 5], n=2, sep=-1), "sep"),
                   (dict(off=[0, 2, 5], n=2, mode=0, plen=2, sep=0), "CONCAT"), (dict(off=[0, 2, 5], n=2, mode=0, plen=0, sep=32), "CONCAT"),
                   (dict(off=[0, 2, 5], n=2, out=None), "out"), (dict(off=[0, 2, 5], n=2, w=None), "words")):
    rc = create(**kw)
    assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), (kw, rc, _lib.last_error())
    assert not h.value
assert lib.latok_detok_info(None, None, None, None, None, None, None, None) == _lib.ERR_INVALID
assert lib.latok_detok_destroy(None) == 0
assert create([0, 2, 5], 2) == _lib.ERR_NOT_INIT and not h.value
assert create([0, 2, 5], 2, mode=0, plen=0, sep=0, p=None) == _lib.ERR_NOT_INIT and not h.value
# the calls: what needs no device first, then the missing device; nothing is written
ip, ids, lens = np.array([0, 3], np.int64), np.array([1, 2, 3], np.int32), np.array([3], np.int32)
out, off, n, unk = np.full(16, 0x5A, np.uint8), np.full(2, -7, np.int64), C.c_int64(0), C.c_int64(0)
skip = np.arange(17, dtype=np.int32)
def csr(flags=0, n_skip=0, cap=16, o=out, n_rows=1, n_pieces=3, n_out=n, indptr=ip):
    return lib.latok_detok_csr(None, indptr.ctypes.data if indptr is not None else None, ids.ctypes.data, n_rows, n_pieces, skip.ctypes.data, n_skip,
                               o.ctypes.data if o is not None else None, cap, off.ctypes.data, C.byref(n_out) if n_out is not None else None, C.byref(unk), flags, None)
def padded(flags=0, n_skip=0, cap=16, o=out, n_rows=1, L=3, n_out=n):
    return lib.latok_detok_padded(None, ids.ctypes.data, lens.ctypes.data, n_rows, L, skip.ctypes.data, n_skip, o.ctypes.data if o is not None else None, cap,
                                  off.ctypes.data, C.byref(n_out) if n_out is not None else None, C.byref(unk), flags, None)
for call in (csr, padded):
    for kw, needle in ((dict(flags=4), "flag"), (dict(flags=64), "flag"), (dict(flags=1 << 20), "flag"), (dict(n_skip=17), "n_skip"), (dict(n_skip=-1), "n_skip"),
                       (dict(cap=-1), "capacity"), (dict(o=None), "size query"), (dict(n_rows=-1), "n_rows"), (dict(n_out=None), "total-size")):
        rc = call(**kw)
        assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), (call.__name__, kw, rc, _lib.last_error())
assert csr(n_pieces=-1) == _lib.ERR_INVALID and csr(indptr=None) == _lib.ERR_INVALID and csr(n_rows=0) == _lib.ERR_INVALID
assert padded(L=-1) == _lib.ERR_INVALID and "max_length" in _lib.last_error()
assert csr() == _lib.ERR_NOT_INIT and padded() == _lib.ERR_NOT_INIT and csr(n_skip=16) == _lib.ERR_NOT_INIT
assert (out == 0x5A).all() and (off == -7).all()
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
for kw in (dict(mode="bpe"), dict(mode="wordpiece", prefix=b"123456789"), dict(mode="wordpiece", sep=b"ab"), dict(ids=[1]), dict(ids=[1 << 31, 0])):
    try:
        batch.Detokenizer([b"a", "b"], **kw)
        raise SystemExit("no ValueError for %%r" %% (kw,))
    except ValueError:
        pass
fake = batch.Detokenizer.__new__(batch.Detokenizer)
fake.handle = None
for call in (lambda: batch.decode_csr(fake, [0, 1], [1]), lambda: batch.decode_batch(None, [[1]]), lambda: batch.decode_padded(fake, np.zeros((1, 2), np.int32)),
             lambda: batch.decode_batch(batch.BPE.__new__(batch.BPE), [[1]])):
    try:
        call()
        raise SystemExit("no ValueError for the decoder")
    except ValueError as e:
        assert "detok" in str(e)
for call in (lambda: batch.decode_csr(fake, [0, 1], [1], errors="replace"), lambda: batch.decode_csr(fake, [0, 1], [1], skip_ids=range(17)),
             lambda: batch.decode_csr(fake, [0, 1], [1], skip_ids=[1 << 31]), lambda: batch.decode_csr(fake, [0, 1], [1.5]),
             lambda: batch.decode_csr(fake, [[0, 1]], [1]), lambda: batch.decode_padded(fake, np.zeros(3, np.int32)),
             lambda: batch.decode_padded(fake, np.zeros((2, 2), np.int32), lengths=[1]),
             lambda: batch.decode_padded(fake, np.zeros((2, 2), np.int32), lengths=[1, 1], attention_mask=np.ones((2, 2))),
             lambda: batch.decode_padded(fake, np.zeros((2, 2), np.int32), attention_mask=np.ones((2, 3)))):
    try:
        call()
        raise SystemExit("no ValueError")
    except ValueError as e:
        assert "detok must" not in str(e), e
try:
    batch.Detokenizer([b"a", "b"], ids=[5, -5], mode="wordpiece", prefix="##", sep=" ")
    raise SystemExit("no RuntimeError")
except RuntimeError:
    pass
print("ok")
""" % ROOT
    env = dict(os.environ, LATOK_DEVICE="4095")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_the_file_loaders_read_what_the_encoders_loaders_read(tmp_path, monkeypatch):
    import base64
    from latok_amd import batch
    made = []
    monkeypatch.setattr(batch.Detokenizer, "__init__", lambda self, w, ids=None, **kw: made.append((list(w), None if ids is None else list(ids), kw)))
    words = [b"a", bytes([0, 255, 10]), b"\n", b"  ", b"abc"]
    order = [3, 0, 4, 1, 2]
    path = tmp_path / "t.tiktoken"
    path.write_bytes(b"".join(base64.b64encode(words[i]) + b" %d\n" % i for i in order) + b"\n")
    batch.Detokenizer.from_tiktoken_file(str(path))
    assert made[-1] == ([words[i] for i in order], order, {})
    for bad in (b"YQ== 0\nYg==\n", b"YQ== 0\n!!! 1\n", b"YQ== zero\n"):
        path.write_bytes(bad)
        with pytest.raises(ValueError):
            batch.Detokenizer.from_tiktoken_file(str(path))
    vocab = tmp_path / "vocab.txt"
    vocab.write_bytes(b"[PAD]\n[CLS]\r\nun\n##able\n\n##\xc3\xa9\n")
    batch.Detokenizer.from_vocab_file(str(vocab), sep=b"_")
    assert made[-1] == ([b"[PAD]", b"[CLS]", b"un", b"##able", b"", b"##\xc3\xa9"], None, dict(mode="wordpiece", prefix=b"##", sep=b"_"))
    assert len(made) == 2
