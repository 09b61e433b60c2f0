"""WordPiece (include/latok_hip.h: latok_wordpiece_*), the parts that need no device: the entry points exist in the library, the
header and latok_amd/_lib.py with one arity and the header stays C99; wordpiece.h, compiled by g++ (once more with the address and
undefined-behaviour sanitizers, as a stand-alone program), builds its two tables and cuts tokens at every alignment inside a
poisoned buffer exactly as tests/helpers/wordpiece_ref.py -- a plain restatement of the definition over bytes and a dict -- does:
random vocabularies, crafted hash collisions at a piece, a damaged table, the empty prefix, V = 0; the reference itself is held to
the `tokenizers` package where that is installed; latok_wordpiece_create refuses bad arguments before it asks for a device."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import pytest

from helpers import murmur3_collide as mc
from helpers import wordpiece_ref as ref
from helpers.murmur3_ref import SEEDS, murmur3_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"latok_wordpiece_create": 9, "latok_wordpiece_destroy": 1, "latok_wordpiece_info": 11,
           "latok_wordpiece_ids_utf8_bytes_batch": 14, "latok_wordpiece_padded_utf8_bytes_batch": 16}
UNK = -1
# the vocabulary and the cases of the issue, checked there against tokenizers.models.WordPiece
ISSUE_WORDS = ["[UNK]", "un", "##aff", "##able", "##ing", "é", "##é", "a", "##b", "unaffable"]
ISSUE_CASES = [("unaff", 100, [("un", 0, 2), ("##aff", 2, 5)]), ("abé", 100, [("a", 0, 1), ("##b", 1, 2), ("##é", 2, 4)]),
               ("ing", 100, [("[UNK]", 0, 3)]), ("abx", 100, [("[UNK]", 0, 3)]), ("unaffablex", 100, [("[UNK]", 0, 10)]),
               ("unaffable", 100, [("unaffable", 0, 9)]), ("éééé", 4, [("é", 0, 2), ("##é", 2, 4), ("##é", 4, 6), ("##é", 6, 8)]),
               ("ééééé", 4, [("[UNK]", 0, 10)])]


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
            elif "*" in a:
                assert b is C.c_void_p or issubclass(b, C._Pointer), (name, a, b)
            else:
                assert b is (C.c_int64 if a.startswith("int64_t") else C.c_int), (name, a, b)
    assert "latok_debug_wordpiece_limits" in exported
    for name in ("WordPiece", "wordpiece_ids_utf8_csr", "wordpiece_ids_utf8_batch", "wordpiece_ids_batch", "wordpiece_encode_utf8_batch"):
        assert callable(getattr(batch, name)), name
    assert callable(batch.WordPiece.from_vocab_file)
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    comment = text[:text.index("typedef struct latok_wordpiece")].rsplit("/*", 1)[1]
    for needle in ("CHAR START", "(b & 0xC0) != 0x80", "LARGEST p", "WHOLE token", "max_chars", "V = 0", "first wins", "PIECES",
                   "latok_token_spans_utf8_bytes_batch", "LATOK_ERR_INVALID", "BasicTokenizer", "BPE", "flow form", "sentence pairs"):
        assert needle in comment, needle


def test_limits_hook():
    from latok_amd import _lib
    import numpy as np
    fn = _lib.load().latok_debug_wordpiece_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(4, np.int64)
    assert fn(out.ctypes.data, 4) == 4
    assert out[0] > 0 and out[1] > 0 and out[2] == 8 and out[3] == 1024


def test_header_with_the_new_calls_is_c99_and_the_example_compiles(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "latok_hip.h"\n'
                   "int f(const uint8_t* u, const int64_t* o, int64_t* ip, int64_t* sp, int32_t* ids, int32_t* len, int64_t* n) {\n"
                   "    latok_wordpiece* w = NULL;\n"
                   "    int64_t a, b, c, d, e; uint8_t pre[8]; int pl, mc, dev; uint32_t seed;\n"
                   '    int rc = latok_wordpiece_create(u, o, 1, NULL, (const uint8_t*)"##", 2, 100, 7u, &w);\n'
                   "    rc += latok_wordpiece_info(w, &a, &b, &c, &d, &e, pre, &pl, &mc, &seed, &dev);\n"
                   "    rc += latok_wordpiece_ids_utf8_bytes_batch(u, o, 1, -1, w, -1, ip, ids, sp, 64, n, NULL, 0, NULL);\n"
                   "    rc += latok_wordpiece_padded_utf8_bytes_batch(u, o, 1, -1, w, 0, 16, 1, 101, 102, 0, ids, len, n, 0, NULL);\n"
                   "    return rc + latok_wordpiece_destroy(w);\n}\n")
    strict = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c"]
    subprocess.check_call(strict + [str(src), "-o", str(tmp_path / "use.o")])
    subprocess.check_call(strict + [os.path.join(ROOT, "examples", "wordpiece_utf8.c"), "-o", str(tmp_path / "example.o")])


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_the_reference_gives_the_cases_of_the_issue():
    d = ref.vocab_dict([w.encode() for w in ISSUE_WORDS])
    for word, max_chars, want in ISSUE_CASES:
        got = ref.cut(word.encode(), d, b"##", max_chars, unk=0)
        assert got == [(ISSUE_WORDS.index(w), a, e) for w, a, e in want], (word, got)


def _random_word(rng, alphabet, n):
    return "".join(rng.choice(alphabet) for _ in range(n))


def test_the_reference_agrees_with_the_tokenizers_package():
    tk = pytest.importorskip("tokenizers")
    rng = random.Random(7)
    alphabet = "abcdeé日🤓"                       # 1-, 2-, 3- and 4-byte chars
    words = ["[UNK]"] + sorted({_random_word(rng, alphabet, rng.randint(1, 4)) for _ in range(60)} |
                               {"##" + _random_word(rng, alphabet, rng.randint(1, 3)) for _ in range(60)})
    vocab = {w: i for i, w in enumerate(words)}
    d = ref.vocab_dict([w.encode() for w in words])
    probes = [_random_word(rng, alphabet, rng.randint(1, 9)) for _ in range(600)] + [w for w in words if not w.startswith(("##", "["))]
    probes += [w for w, _, _ in ISSUE_CASES]
    n_multi = 0
    for max_chars in (100, 4, 1):
        model = tk.models.WordPiece(vocab=vocab, unk_token="[UNK]", max_input_chars_per_word=max_chars)
        for word in probes:
            got = ref.cut(word.encode(), d, b"##", max_chars, unk=0)
            want = [(t.id, t.offsets[0], t.offsets[1]) for t in model.tokenize(word)]
            assert got == want, (word, max_chars, got, want)
            n_multi += len(got) > 1
    assert n_multi > 100
    model = tk.models.WordPiece(vocab={w: i for i, w in enumerate(ISSUE_WORDS)}, unk_token="[UNK]", max_input_chars_per_word=4)
    for word, max_chars, want in ISSUE_CASES:
        if max_chars == 4:
            assert [(t.value, t.offsets[0], t.offsets[1]) for t in model.tokenize(word)] == want


# ---- wordpiece.h on the host -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    """the stand-alone program, built by plain g++ and once more with -fsanitize=address,undefined; it is run directly"""
    exe = tmp_path_factory.mktemp("wordpiece_" + request.param) / "wordpiece_harness"
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "wordpiece_harness.cpp"), "-o", str(exe)])

    def run(script, poison=0xA5):
        out = subprocess.run([str(exe)], input="%02x\n" % poison + script, capture_output=True, text=True)
        assert out.returncode == 0, ({2: "a text load left the token's dwords", 3: "a table load left the table",
                                      4: "the counting walk and the emitting walk disagree"}.get(out.returncode, out.returncode), out.stderr[-2000:])
        return out.stdout.splitlines()

    return run


def _run(harness, words, tokens, prefix=b"##", max_chars=100, seed=0, ids=None, unk=UNK, pads=(0, 1, 2, 3), damaged=False,
         poisons=(0x00, 0xFF, 0xA5)):
    """every token at every pad, against the reference; returns (info of the tables, slot loads per case)"""
    d = ref.vocab_dict(words, ids)
    cases = [(pad, t) for t in tokens for pad in pads]
    lines = ["V %x %s %d %d" % (seed, prefix.hex() or "-", max_chars, len(words))]
    lines += ["%s %s" % ("-" if ids is None else ids[i], w.hex() or "-") for i, w in enumerate(words)]
    lines += ["F"] if damaged else []
    lines += ["T %d %d %s" % (pad, unk, t.hex()) for pad, t in cases]
    info = loads = None
    for poison in poisons:      # what surrounds the token in its dwords must not reach the hash, the compare or the char count
        out = harness("\n".join(lines) + "\n", poison)
        m = re.match(r"slots (\d+) (\d+) used (\d+) (\d+) max (\d+) (\d+)$", out[0])
        assert m and len(out) == 1 + len(cases), out[:3]
        info = tuple(map(int, m.groups()))
        cont = {w[len(prefix):] for w in d if w.startswith(prefix) and len(w) > len(prefix)}
        assert info[2] == len([w for w in d if w]) and info[3] == len(cont)
        assert info[4] == max([len(w) for w in words] + [0]) and info[5] == max([len(w) for w in cont] + [0])
        loads = []
        for (pad, t), line in zip(cases, out[1:]):
            f = line.split()
            got = [tuple(map(int, x.split(":"))) for x in f[1:-1]]
            want = [(unk, 0, len(t))] if damaged else ref.cut(t, d, prefix, max_chars, unk)
            assert int(f[0]) == len(got) and got == want, (poison, pad, t, got, want)
            loads.append(int(f[-1]))
    return info, loads


def test_the_cases_of_the_issue(harness):
    words = [w.encode() for w in ISSUE_WORDS]
    for max_chars in (100, 4):
        _run(harness, words, [w.encode() for w, _, _ in ISSUE_CASES], max_chars=max_chars, unk=0, pads=range(8))


def test_every_outcome_of_the_cut(harness):
    words = [b"a", b"##a", b"ab", b"##b", b"##bc", b"abc", b"##x", b"##", b"##y##", b"#", b"###", b"h\xc3", b"##\xa9", b"\xc3"]
    tokens = [b"a", b"ab", b"abc", b"abcb", b"aa", b"aaaa", b"a" * 100, b"a" * 101, b"x", b"ax", b"abx", b"abq", b"abbq", b"abcbq", b"q",
              b"##x", b"##", b"#", b"###", b"a##", b"ay##", b"h\xc3\xa9", b"\xc3\xa9", b"\xc3", b"a\xa9", b"\xa9", b"a\xc3", b"abcd" * 40]
    _run(harness, words, tokens)
    _run(harness, words, tokens, max_chars=3)
    _run(harness, words, tokens, ids=[5, -3, 7, 0x7FFFFFFF, -0x80000000, 0, 0, 1, 2, 3, 4, 9, 9, 10], unk=-7, seed=0x9747B28C)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_vocabularies_and_words(harness, seed):
    rng = random.Random(seed)
    alphabets = [b"ab", b"abc#", bytes([0x61, 0x62, 0xC3, 0xA9, 0xE6, 0x97, 0xA5, 0xF0, 0x9F, 0xA4, 0x93, 0x23])]
    for alphabet in alphabets:
        for prefix in (b"##", b"", b"#", b"\xc3", b"ab##ab##"):
            words = [bytes(rng.choice(alphabet) for _ in range(rng.randint(0, 5))) for _ in range(rng.choice((3, 40, 200)))]
            words += [prefix + bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 4))) for _ in range(len(words))]
            rng.shuffle(words)
            tokens = [bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 14))) for _ in range(150)]
            tokens += [w for w in words if w][:40]
            for max_chars in (100, 5):
                _run(harness, words, tokens, prefix=prefix, max_chars=max_chars, seed=seed, pads=(0, 1, 2, 3, 6), poisons=(0xA5, 0xFF))


def test_max_chars_counts_chars_not_bytes(harness):
    for ch in (b"a", "é".encode(), "日".encode(), "🤓".encode()):
        words = [ch, b"##" + ch]
        for m in (1, 2, 7, 100, 1024):
            info, _ = _run(harness, words, [ch * m, ch * (m + 1), ch * m + b"\x80" * 3, b"\x80" + ch * m], max_chars=m, pads=(0, 3))
            assert info[4] == len(ch) + 2


def test_long_tokens_do_not_hash_their_whole_length_per_end(harness):
    words = [b"ab", b"##cd"]
    _, loads = _run(harness, words, [b"q" * 1000, b"ab" + b"q" * 1000, b"ab" + b"cd" * 40], max_chars=1024, pads=(1,), poisons=(0xA5,))
    # the candidates of a piece are no longer than the table's longest word (2 bytes): at most 2 probes for the piece that misses,
    # whatever the token's length; a probe of these near-empty tables takes 1 to 3 slot loads; every token is walked twice
    assert 0 < loads[0] <= 2 * 2 * 3 and 0 < loads[1] <= 2 * (1 + 2) * 3 and 0 < loads[2] <= 2 * 41 * 3, loads


@pytest.mark.parametrize("seed", SEEDS)
def test_crafted_collisions_at_a_piece_are_told_apart_by_their_bytes(harness, seed):
    rng = random.Random(seed)
    pairs = []
    for n in (5, 6, 7, 8, 9, 11, 12, 13, 16, 17, 23):
        a = bytes(rng.randrange(0x61, 0x7B) for _ in range(n))
        pairs += [(a, mc.collide(a, seed, w)) for w in mc.positions(n)[:3]]
    if seed == 0:
        pairs += list(mc.KNOWN_WORD_PAIRS)
    assert len(pairs) > 15 and all(murmur3_ref(a, seed) == murmur3_ref(b, seed) and a != b and len(a) == len(b) for a, b in pairs)
    # the vocabulary holds a (as a word and as a continuation); the candidate piece b has a's hash and a's length, at either place
    words = [b"un"] + [a for a, _ in pairs] + [b"##" + a for a, _ in pairs]
    tokens = [b for _, b in pairs] + [b"un" + b for _, b in pairs] + [a for a, _ in pairs] + [b"un" + a for a, _ in pairs]
    _run(harness, words, tokens, seed=seed)
    both = [w for p in pairs for w in p]
    _run(harness, both + [b"##" + w for w in both] + [b"un"], both + [b"un" + w for w in both], seed=seed, pads=(0, 3))


def test_a_table_without_an_empty_slot_ends_every_loop(harness):
    words = [b"w%d" % i for i in range(40)] + [b"##w%d" % i for i in range(40)]
    info, loads = _run(harness, words, [b"w1", b"w1w2", b"other", b"w" * 50], damaged=True, unk=-5, pads=(0, 3))
    # every probe gave up after n_slots steps: one per candidate end, at most max_len ends for the first piece, twice (count, emit)
    assert all(l % info[0] == 0 and 0 < l <= 2 * info[4] * info[0] for l in loads), (info, loads)


def test_the_empty_prefix(harness):
    words = [b"ab", b"c", b"abc", b"d"]
    info, _ = _run(harness, words, [b"abc", b"abcd", b"cab", b"dd", b"abab", b"abx", b"xab", b"cabcd"], prefix=b"")
    assert info[2] == info[3] == 4


def test_an_empty_vocabulary_and_empty_words(harness):
    _run(harness, [], [b"a", b"ab", b"\xc3\xa9", b"a" * 300])
    _run(harness, [b"", b"##", b""], [b"a", b"##", b"#"])


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_create_refuses_bad_arguments_before_it_asks_for_a_device():
    code = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import _lib
lib = _lib.load()
words = np.frombuffer(b"abcde", np.uint8)
pre = np.frombuffer(b"##", np.uint8)
h = C.c_void_p()
def create(off, n, out=h, w=words, plen=2, mc=100, p=pre):
    off = np.array(off, np.int64)
    return lib.latok_wordpiece_create(w.ctypes.data if w is not None else None, off.ctypes.data, n, None, p.ctypes.data if p is not None else None,
                                      plen, mc, 0, C.byref(out) if out is not None else None)
for kw, needle in ((dict(off=[1, 2, 5], n=2), "start at 0"), (dict(off=[0, 3, 2], n=2), "non-decreasing"), (dict(off=[0, 2, 5], n=-1), "n_words"),
                   (dict(off=[0, 2, 5], n=1 << 31), "n_words"), (dict(off=[0, 1 << 32], n=1), "2^32"), (dict(off=[0, 2, 5], n=2, plen=9), "prefix_len"),
                   (dict(off=[0, 2, 5], n=2, plen=-1), "prefix_len"), (dict(off=[0, 2, 5], n=2, mc=0), "max_chars"),
                   (dict(off=[0, 2, 5], n=2, mc=1025), "max_chars"), (dict(off=[0, 2, 5], n=2, p=None), "prefix"),
                   (dict(off=[0, 2, 5], n=2, out=None), "wp_out"), (dict(off=[0, 2, 5], n=2, w=None), "words")):
    rc = create(**kw)
    assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), (kw, rc, _lib.last_error())
    assert not h.value
assert lib.latok_wordpiece_info(None, None, None, None, None, None, None, None, None, None, None) == _lib.ERR_INVALID
assert lib.latok_wordpiece_destroy(None) == 0
assert create([0, 2, 5], 2) == _lib.ERR_NOT_INIT and not h.value
assert create([0, 2, 5], 2, plen=0, p=None) == _lib.ERR_NOT_INIT and not h.value
# the calls: a stray flag bit first, then the missing device; nothing is written
u8, boff = np.frombuffer(b"abc def", np.uint8), np.array([0, 7], np.int64)
ids, ip, n = np.full(8, 0x5A5A5A5A, np.int32), np.full(2, -7, np.int64), C.c_int64(0)
for flags in (4, 64, 1 << 20):
    rc = lib.latok_wordpiece_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, None, -1, ip.ctypes.data, ids.ctypes.data, None, 8, C.byref(n), None, flags, None)
    assert rc == _lib.ERR_INVALID and "flag" in _lib.last_error(), rc
    rc = lib.latok_wordpiece_padded_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, None, -1, 8, 1, 1, 2, 0, ids.ctypes.data, ip.ctypes.data, None, flags, None)
    assert rc == _lib.ERR_INVALID and "flag" in _lib.last_error(), rc
rc = lib.latok_wordpiece_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, None, -1, ip.ctypes.data, ids.ctypes.data, None, 8, C.byref(n), None, 0, None)
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
for kw in (dict(prefix=b"123456789"), dict(max_chars=0), dict(max_chars=1025), dict(max_chars=2.5), dict(seed=-1), dict(ids=[1]), dict(ids=[1 << 31, 0])):
    try:
        batch.WordPiece([b"a", "b"], **kw)
        raise SystemExit("no ValueError for %%r" %% (kw,))
    except ValueError:
        pass
fake = batch.WordPiece.__new__(batch.WordPiece)
fake.handle = None
for call in (lambda: batch.wordpiece_ids_utf8_batch([b"a"], fake), lambda: batch.wordpiece_ids_batch(["a"], None),
             lambda: batch.wordpiece_encode_utf8_batch([b"a"], fake, 8)):
    try:
        call()
        raise SystemExit("no ValueError for the vocabulary")
    except ValueError as e:
        assert "wp" in str(e)
for kw in (dict(max_length=0), dict(max_length=2, cls_id=1, sep_id=2), dict(max_length=8, cls_id=1), dict(max_length=8, unk_id=1 << 31),
           dict(max_length=8, pad_id=None)):
    try:
        batch.wordpiece_encode_utf8_batch([b"a"], fake, **kw)
        raise SystemExit("no ValueError for %%r" %% (kw,))
    except ValueError:
        pass
try:
    batch.WordPiece([b"a", "b"], ids=[5, -5], seed=7)
    raise SystemExit("no RuntimeError")
except RuntimeError:
    pass
print("ok")
""" % ROOT
    env = dict(os.environ, LATOK_DEVICE="4095")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)
