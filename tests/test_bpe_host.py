"""Byte-level BPE (include/latok_hip.h: latok_bpe_*), the parts that need no device: the entry points exist in the library, the header
and latok_amd/_lib.py with one arity and the header stays C99; bpe.h, compiled by g++ (once more with the address and
undefined-behaviour sanitizers, as a stand-alone program), builds its table and cuts tokens at every alignment inside a poisoned buffer
exactly as tests/helpers/bpe_ref.py -- a plain restatement of the definition over bytes and a dict -- does: the worked table, random
vocabularies over small alphabets, every length 1 .. 70, crafted hash collisions at a pair, a damaged table, V = 0, duplicates; a
counter in the harness proves the lookup bound; the reference itself is held to the `tiktoken` package where that is installed;
latok_bpe_create refuses bad arguments before it asks for a device."""
import base64
import ctypes as C
import os
import random
import re
import subprocess
import sys

import pytest

from helpers import bpe_ref as ref
from helpers import murmur3_collide as mc
from helpers.murmur3_ref import SEEDS, murmur3_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"latok_bpe_create": 8, "latok_bpe_destroy": 1, "latok_bpe_info": 8, "latok_bpe_ids_utf8_bytes_batch": 14,
           "latok_bpe_padded_utf8_bytes_batch": 16}
UNK = -1


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
    assert "latok_debug_bpe_limits" in exported
    for name in ("BPE", "bpe_ids_utf8_csr", "bpe_ids_utf8_batch", "bpe_ids_batch", "bpe_encode_utf8_batch"):
        assert callable(getattr(batch, name)), name
    assert callable(batch.BPE.from_tiktoken_file)
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    comment = text[:text.index("typedef struct latok_bpe")].rsplit("/*", 1)[1]
    for needle in ("RANK", "first wins", "lead_space", "0x20", "L > max_bytes", "shortcut", "LOWEST rank", "LEFTMOST", "NOT withdrawn", "V = 0",
                   "PIECES", "latok_token_spans_utf8_bytes_batch", "LATOK_ERR_INVALID", "tiktoken", "regex pre-tokenizer", "merges.txt",
                   "Unigram", "flow form", "decoding"):
        assert needle in comment, needle


def test_limits_hook():
    from latok_amd import _lib
    import numpy as np
    fn = _lib.load().latok_debug_bpe_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(4, np.int64)
    assert fn(out.ctypes.data, 4) == 4
    assert out[0] > 0 and out[0] % 64 == 0 and out[1] > 0 and out[2] == 64 and out[3] == 4096
    assert fn(out.ctypes.data, 2) == 2 and fn(None, 4) < 0


def test_header_with_the_new_calls_is_c99_and_the_example_compiles(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "latok_hip.h"\n'
                   "int f(const uint8_t* u, const int64_t* o, int64_t* ip, int64_t* sp, int32_t* ids, int32_t* len, int64_t* n) {\n"
                   "    latok_bpe* w = NULL;\n"
                   "    int64_t a, b, c; int mb, ls, dev; uint32_t seed;\n"
                   "    int rc = latok_bpe_create(u, o, 1, NULL, 4096, 1, 7u, &w);\n"
                   "    rc += latok_bpe_info(w, &a, &b, &c, &mb, &ls, &seed, &dev);\n"
                   "    rc += latok_bpe_ids_utf8_bytes_batch(u, o, 1, -1, w, -1, ip, ids, sp, 64, n, NULL, 0, NULL);\n"
                   "    rc += latok_bpe_padded_utf8_bytes_batch(u, o, 1, -1, w, 0, 16, 1, 101, 102, 0, ids, len, n, 0, NULL);\n"
                   "    return rc + latok_bpe_destroy(w);\n}\n")
    strict = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c"]
    subprocess.check_call(strict + [str(src), "-o", str(tmp_path / "use.o")])
    subprocess.check_call(strict + [os.path.join(ROOT, "examples", "bpe_utf8.c"), "-o", str(tmp_path / "example.o")])


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_the_reference_gives_the_worked_cases():
    d = ref.rank_dict(ref.WORKED_WORDS)
    assert len(d) == 15 and d[b"b"] == 1
    for token, max_bytes, want in ref.WORKED_CASES:
        assert ref.cut(token, d, max_bytes, unk=-1) == want, token
    # greedy longest-prefix would give (bc)(d): the rule is rank, not position
    assert ref.cut(b"bcd", d) != [(6, 0, 2), (3, 2, 3)]
    assert ref.cut(b"ab", {}, unk=-9) == [(-9, 0, 1), (-9, 1, 2)] and ref.cut(b"abc", {}, 2, unk=-9) == [(-9, 0, 3)]


def test_the_trainer_makes_merges_the_reference_reaches():
    rng = random.Random(3)
    corpus = [bytes(rng.choice(b"abc") for _ in range(rng.randint(1, 9))) for _ in range(300)]
    words = ref.train(corpus, 40)
    assert words[:3] == [b"a", b"b", b"c"] and len(words) == 43 and len(set(words)) == 43
    d = ref.rank_dict(words)
    assert all(len(w) == 1 or any(w[:i] in d and w[i:] in d for i in range(1, len(w))) for w in words)
    assert sum(len(ref.cut(t, d)) < len(t) for t in corpus) > 200


def test_the_reference_agrees_with_the_tiktoken_package():
    tiktoken = pytest.importorskip("tiktoken")
    singles = [bytes([b]) for b in range(256)]
    words = [w for w in ref.WORKED_WORDS[:-1]] + [s for s in singles if s not in ref.WORKED_WORDS]
    d = ref.rank_dict(words)
    enc = tiktoken.Encoding("worked", pat_str=r"[\s\S]+", mergeable_ranks=dict(d), special_tokens={})
    rng = random.Random(11)
    probes = [t for t, _, _ in ref.WORKED_CASES] + [bytes(rng.choice(b"abcd \xc3\xa9x") for _ in range(rng.randint(1, 12))) for _ in range(500)]
    for t in probes:
        assert [p[0] for p in ref.cut(t, d)] == enc.encode_single_piece(t), t


# ---- bpe.h on the host -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    """the stand-alone program, built by plain g++ and once more with -fsanitize=address,undefined; it is run directly"""
    exe = tmp_path_factory.mktemp("bpe_" + request.param) / "bpe_harness"
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "bpe_harness.cpp"), "-o", str(exe)])

    def run(script, poison=0xA5):
        out = subprocess.run([str(exe)], input="%02x\n" % poison + script, capture_output=True, text=True)
        assert out.returncode == 0, ({2: "a text load left the token's dwords", 3: "a table load left the table",
                                      4: "the lane state and the wide state disagree"}.get(out.returncode, out.returncode), out.stderr[-2000:])
        return out.stdout.splitlines()

    return run


def _run(harness, words, tokens, max_bytes=4096, seed=0, ids=None, unk=UNK, pads=(0, 1, 2, 3), damaged=False, poisons=(0x00, 0xFF, 0xA5)):
    """every token at every pad, against the reference and the lookup bound; returns (info of the table, slot loads per case)"""
    d = ref.rank_dict(words)
    cases = [(pad, t) for t in tokens for pad in pads]
    lines = ["V %x %d %d" % (seed, max_bytes, len(words))]
    lines += ["%s %s" % ("-" if ids is None else ids[i], w.hex() or "-") for i, w in enumerate(words)]
    lines += ["F"] if damaged else []
    lines += ["T %d %d %s" % (pad, unk, t.hex()) for pad, t in cases]
    info = loads = None
    for poison in poisons:      # what surrounds the token in its dwords must not reach the hash or the compare
        out = harness("\n".join(lines) + "\n", poison)
        m = re.match(r"slots (\d+) used (\d+) max (\d+)$", out[0])
        assert m and len(out) == 1 + len(cases), out[:3]
        info = tuple(map(int, m.groups()))
        assert info[1] == len(d) and info[2] == max([len(w) for w in words] + [0])
        loads = []
        for (pad, t), line in zip(cases, out[1:]):
            f = line.split()
            got = [tuple(map(int, x.split(":"))) for x in f[1:-3]]
            if damaged:
                want = [(unk, 0, len(t))] if len(t) > max_bytes else [(unk, i, i + 1) for i in range(len(t))]
            else:
                want = ref.cut(t, d, max_bytes, unk, ids)
            assert int(f[0]) == len(got) and got == want, (poison, pad, t, got, want)
            lookups, n_merges = int(f[-3]), int(f[-2])
            if not damaged:
                assert n_merges == ref.merges(t, d, max_bytes), (t, n_merges)
            # every initial pair once, two new pairs per merge, one lookup per part, the whole token
            one_piece = len(t) > max_bytes or (t in d and not damaged)
            assert lookups <= (1 if one_piece else (len(t) - 1) + 2 * n_merges + len(got) + 1), (t, lookups, n_merges, len(got))
            loads.append(int(f[-1]))
    return info, loads


def test_the_worked_table(harness):
    for max_bytes in (4096, 2):
        _run(harness, ref.WORKED_WORDS, [t for t, _, _ in ref.WORKED_CASES] + [b" a", b" ", b"  ", b"dcba", b"abcdabcd", b"ab" * 40, b"ad" * 40],
             max_bytes=max_bytes, pads=range(8))
    d = ref.rank_dict(ref.WORKED_WORDS)
    for token, max_bytes, want in ref.WORKED_CASES:     # the table of the definition itself, not only the reference
        out = harness("V 0 %d %d\n" % (max_bytes, len(ref.WORKED_WORDS)) + "".join("- %s\n" % w.hex() for w in ref.WORKED_WORDS) +
                      "T 1 -1 %s\n" % token.hex())
        assert [tuple(map(int, x.split(":"))) for x in out[1].split()[1:-3]] == want, token
    assert d[b"adc"] == 14


@pytest.mark.parametrize("seed", SEEDS)
def test_random_vocabularies_over_small_alphabets(harness, seed):
    rng = random.Random(seed)
    for alphabet in (b"abc", b"abcd", b"ab\xc3\xa9"):
        for n_words in (3, 30, 200):
            words = [bytes(rng.choice(alphabet) for _ in range(rng.choice((1, 1, 2, 2, 2, 3, 3, 4, 5)))) for _ in range(n_words)]
            tokens = [bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 20))) for _ in range(120)] + [w for w in words][:30]
            ids = [rng.randrange(-1 << 31, 1 << 31) for _ in words] if n_words == 30 else None
            _run(harness, words, tokens, seed=seed, ids=ids, unk=-7 if ids else UNK, pads=(0, 1, 2, 3, 6), poisons=(0xA5, 0xFF))
        corpus = [bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 12))) for _ in range(200)]
        trained = ref.train(corpus, 60)
        _run(harness, trained, corpus[:80] + [bytes(rng.choice(alphabet) for _ in range(rng.randint(60, 300))) for _ in range(6)], seed=seed,
             pads=(0, 3), poisons=(0xA5,))


def test_every_length_at_every_alignment(harness):
    rng = random.Random(5)
    corpus = [bytes(rng.choice(b"abc") for _ in range(rng.randint(1, 10))) for _ in range(300)]
    words = ref.train(corpus, 50)
    tokens = [bytes(rng.choice(b"abc") for _ in range(n)) for n in range(1, 71) for _ in range(2)]
    tokens += [b"ab" * 32, b"ab" * 33, b"a" * 64, b"a" * 65, b"abc" * 21 + b"a"]
    _run(harness, words, tokens)
    _run(harness, ref.WORKED_WORDS, [(b"ab" * 40)[:n] for n in range(1, 71)] + [(b"ad" * 40)[:n] for n in range(60, 71)])


def test_max_bytes_and_long_tokens(harness):
    words = ref.WORKED_WORDS
    for mb in (1, 2, 3, 64, 65, 4096):
        _run(harness, words, [(b"ab" * 2050)[:n] for n in (mb - 1, mb, mb + 1) if n > 0], max_bytes=mb, pads=(0, 3), poisons=(0xA5,))
    # the most rounds possible (every pair of the token merges) and none at all
    _, loads = _run(harness, words, [b"ab" * 2048, b"ad" * 2048, b"x" * 4096], pads=(1,), poisons=(0xA5,))
    assert all(l > 0 for l in loads)
    # a span longer than the longest word needs no probe: an unknown long token costs its initial pairs and its parts
    _run(harness, [b"a", b"b"], [b"ab" * 100], pads=(0,), poisons=(0xA5,))


@pytest.mark.parametrize("seed", SEEDS)
def test_crafted_collisions_at_a_pair_are_told_apart_by_their_bytes(harness, seed):
    rng = random.Random(seed)
    pairs = []
    for n in (5, 6, 7, 8, 9, 11, 12, 13, 16, 17, 23):
        a = bytes(rng.randrange(0x61, 0x7B) for _ in range(n))
        pairs += [(a, mc.collide(a, seed, w)) for w in mc.positions(n)[:3]]
    if seed == 0:
        pairs += list(mc.KNOWN_WORD_PAIRS)
    assert len(pairs) > 15 and all(murmur3_ref(a, seed) == murmur3_ref(b, seed) and a != b and len(a) == len(b) for a, b in pairs)
    for a, b in pairs[:12]:
        # a is reachable by merges: its prefixes are words (ranks ascending); b's prefixes are words up to len - 1, so b's last merge
        # asks for the pair whose bytes have a's hash and a's length but are not a
        k = next(i for i in range(len(a)) if a[i] != b[i])
        singles = sorted({bytes([x]) for x in a + b})
        chain_a = [a[:i] for i in range(2, len(a) + 1)]
        chain_b = [b[:i] for i in range(2, len(b))]
        words = singles + chain_a + [w for w in chain_b if w not in chain_a]
        _run(harness, words, [a, b, b + a, a + b, a[:k + 1] + b[k + 1:]], seed=seed, pads=(0, 1, 3), poisons=(0xA5,))
        _run(harness, words + [b], [a, b, b + a], seed=seed, pads=(0, 2), poisons=(0xA5,))
    # ... and at the whole token (the shortcut's lookup)
    _run(harness, [a for a, _ in pairs], [b for _, b in pairs] + [a for a, _ in pairs], seed=seed)


def test_a_table_without_an_empty_slot_ends_every_loop(harness):
    words = [b"w%d" % i for i in range(40)]
    info, loads = _run(harness, words, [b"w1", b"w1w2", b"other", b"w" * 50], damaged=True, unk=-5, pads=(0, 3))
    # every probe gave up after n_slots steps; a token of L bytes asks for the whole token (if no longer than the longest word),
    # its L - 1 pairs and its L parts
    assert all(l % info[0] == 0 and 0 < l <= 2 * 50 * info[0] for l in loads), (info, loads)


def test_an_empty_vocabulary_empty_words_and_duplicates(harness):
    _run(harness, [], [b"a", b"ab", b"\xc3\xa9", b"a" * 300, b"a" * 5000])
    _run(harness, [b"", b"", b""], [b"a", b"ab"])
    info, _ = _run(harness, [b"a", b"b", b"ab", b"a", b"ab", b"", b"b", b"ba"], [b"ab", b"ba", b"abab", b"baba", b"aab"], ids=[1, 2, 3, 4, 5, 6, 7, 8])
    assert info[1] == 4


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
def create(off, n, out=h, w=words, mb=4096, ls=0):
    off = np.array(off, np.int64)
    return lib.latok_bpe_create(w.ctypes.data if w is not None else None, off.ctypes.data, n, None, mb, ls, 0, C.byref(out) if out is not None else None)
for kw, needle in ((dict(off=[1, 2, 5], n=2), "start at 0"), (dict(off=[0, 3, 2], n=2), "non-decreasing"), (dict(off=[0, 2, 5], n=-1), "n_words"),
                   (dict(off=[0, 2, 5], n=1 << 31), "n_words"), (dict(off=[0, 1 << 32], n=1), "2^32"), (dict(off=[0, 2, 5], n=2, mb=0), "max_bytes"),
                   (dict(off=[0, 2, 5], n=2, mb=4097), "max_bytes"), (dict(off=[0, 2, 5], n=2, mb=-1), "max_bytes"),
                   (dict(off=[0, 2, 5], n=2, ls=2), "lead_space"), (dict(off=[0, 2, 5], n=2, ls=-1), "lead_space"),
                   (dict(off=[0, 2, 5], n=2, out=None), "bpe_out"), (dict(off=[0, 2, 5], n=2, w=None), "words")):
    rc = create(**kw)
    assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), (kw, rc, _lib.last_error())
    assert not h.value
assert lib.latok_bpe_info(None, None, None, None, None, None, None, None) == _lib.ERR_INVALID
assert lib.latok_bpe_destroy(None) == 0
assert create([0, 2, 5], 2) == _lib.ERR_NOT_INIT and not h.value
assert create([0, 2, 5], 2, mb=1, ls=1) == _lib.ERR_NOT_INIT and not h.value
# the calls: a stray flag bit first, then the missing device; nothing is written
u8, boff = np.frombuffer(b"abc def", np.uint8), np.array([0, 7], np.int64)
ids, ip, n = np.full(8, 0x5A5A5A5A, np.int32), np.full(2, -7, np.int64), C.c_int64(0)
for flags in (4, 64, 1 << 20):
    rc = lib.latok_bpe_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, None, -1, ip.ctypes.data, ids.ctypes.data, None, 8, C.byref(n), None, flags, None)
    assert rc == _lib.ERR_INVALID and "flag" in _lib.last_error(), rc
    rc = lib.latok_bpe_padded_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, None, -1, 8, 1, 1, 2, 0, ids.ctypes.data, ip.ctypes.data, None, flags, None)
    assert rc == _lib.ERR_INVALID and "flag" in _lib.last_error(), rc
rc = lib.latok_bpe_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, None, -1, ip.ctypes.data, ids.ctypes.data, None, 8, C.byref(n), None, 0, None)
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
for kw in (dict(max_bytes=0), dict(max_bytes=4097), dict(max_bytes=2.5), dict(max_bytes=True), dict(lead_space=2), dict(lead_space="yes"), dict(seed=-1),
           dict(ids=[1]), dict(ids=[1 << 31, 0])):
    try:
        batch.BPE([b"a", "b"], **kw)
        raise SystemExit("no ValueError for %%r" %% (kw,))
    except ValueError:
        pass
fake = batch.BPE.__new__(batch.BPE)
fake.handle = None
for call in (lambda: batch.bpe_ids_utf8_batch([b"a"], fake), lambda: batch.bpe_ids_batch(["a"], None), lambda: batch.bpe_encode_utf8_batch([b"a"], fake, 8),
             lambda: batch.bpe_ids_utf8_batch([b"a"], batch.WordPiece.__new__(batch.WordPiece))):
    try:
        call()
        raise SystemExit("no ValueError for the vocabulary")
    except ValueError as e:
        assert "bpe" in str(e)
for kw in (dict(max_length=0), dict(max_length=2, bos_id=1, eos_id=2), dict(max_length=8, bos_id=1), dict(max_length=8, unk_id=1 << 31),
           dict(max_length=8, pad_id=None)):
    try:
        batch.bpe_encode_utf8_batch([b"a"], fake, **kw)
        raise SystemExit("no ValueError for %%r" %% (kw,))
    except ValueError:
        pass
try:
    batch.BPE([b"a", "b"], ids=[5, -5], seed=7, lead_space=True, max_bytes=64)
    raise SystemExit("no RuntimeError")
except RuntimeError:
    pass
print("ok")
""" % ROOT
    env = dict(os.environ, LATOK_DEVICE="4095")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_from_tiktoken_file_reads_what_the_test_wrote(tmp_path, monkeypatch):
    from latok_amd import batch
    words = [w for w in ref.WORKED_WORDS[:-1]] + [bytes([0, 255, 10]), b"\n", b"  "]
    made = []
    monkeypatch.setattr(batch.BPE, "__init__", lambda self, w, **kw: made.append((list(w), kw)))
    order = list(range(len(words)))
    random.Random(2).shuffle(order)
    path = tmp_path / "worked.tiktoken"
    path.write_bytes(b"".join(base64.b64encode(words[i]) + b" %d\n" % i for i in order))
    batch.BPE.from_tiktoken_file(str(path), lead_space=True, max_bytes=99)
    assert made == [(words, dict(lead_space=True, max_bytes=99))]
    for bad in (b"YQ== 0\nYg== 2\n", b"YQ== 0\nYg== 0\n", b"YQ== 1\n", b"YQ== 0\nYg==\n", b"YQ== 0\n!!! 1\n", b"YQ== zero\n"):
        path.write_bytes(bad)
        with pytest.raises(ValueError):
            batch.BPE.from_tiktoken_file(str(path))
    assert len(made) == 1
