"""Vocabulary lookup (include/latok_hip.h: latok_vocab_*, latok_token_ids_utf8_bytes_batch, latok_flow_token_ids_utf8_bytes), the
parts that need no device: the entry points exist in the library, the header and latok_amd/_lib.py with one arity and the header
stays C99; vocab_table.h, compiled by g++ (once more with the address and undefined-behaviour sanitizers, as a stand-alone
program), builds tables and probes them for tokens at every alignment inside a poisoned buffer and gives the ids of a Python dict
built by setdefault -- hits, misses, duplicates, the empty word, the wrap at the last slot, crafted hash collisions, a damaged
table; latok_vocab_create refuses bad arguments before it asks for a device; the Python wrappers refuse a bad unk_id likewise;
and the ranges a flow batch notes are the stated ones."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import murmur3_collide as mc
from helpers.murmur3_ref import SEEDS, murmur3_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"latok_vocab_create": 6, "latok_vocab_destroy": 1, "latok_vocab_info": 5, "latok_token_ids_utf8_bytes_batch": 13,
           "latok_flow_token_ids_utf8_bytes": 12}
UNK = -1


def _header_decl(name):
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    m = re.search(r"^int %s\((.*?)\);" % name, text, re.S | re.M)
    assert m, "%s is not declared in include/latok_hip.h" % name
    args = re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " "))
    return [a.strip() for a in args.split(",")]


def hash_wave_bytes():
    """entry 14 of latok_debug_limits (needs no device)"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(15, np.int64)
    assert fn(out.ctypes.data, 15) == 15
    return int(out[14])


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
            if a == "int32_t unk_id":
                assert b is C.c_int32
            elif a == "uint32_t seed":
                assert b is C.c_uint32
            elif "*" in a:
                assert b is C.c_void_p or issubclass(b, C._Pointer), (name, a, b)
            else:
                assert b is (C.c_int64 if a.startswith("int64_t") else C.c_int), (name, a, b)
    assert "latok_debug_flow_ids_ranges" in exported
    for name in ("Vocab", "token_ids_utf8_csr", "token_ids_utf8_batch", "token_ids_batch", "flow_token_ids_utf8_bytes"):
        assert callable(getattr(batch, name)), name
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    comment = text[:text.index("typedef struct latok_vocab")].rsplit("/*", 1)[1]
    for needle in ("ids_out[rank(s, k)]", "unk_id", "LOWEST index", "first occurrence wins", "never matches", "V = 0",
                   "latok_token_spans_utf8_bytes_batch", "default_tokenizer.py:149-160", "LATOK_ERR_INVALID", "latok_ctx_destroy"):
        assert needle in comment, needle


def test_header_with_the_new_calls_is_c99_and_the_example_compiles(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "latok_hip.h"\n'
                   "int f(const uint8_t* u, const int64_t* o, int64_t* c, int64_t* sp, int32_t* ids, int64_t* n, int64_t* r) {\n"
                   "    latok_vocab* v = NULL;\n"
                   "    int64_t nw, ns; uint32_t seed; int dev;\n"
                   "    int rc = latok_vocab_create(u, o, 1, NULL, 7u, &v) + latok_vocab_info(v, &nw, &ns, &seed, &dev);\n"
                   "    rc += latok_token_ids_utf8_bytes_batch(u, o, 1, -1, v, -1, c, sp, ids, 64, n, 0, NULL);\n"
                   "    rc += latok_token_ids_utf8_bytes_batch(u, o, 1, -1, v, 0x7fffffff, NULL, NULL, ids, 64, n, LATOK_OUT_INT32, NULL);\n"
                   "    rc += latok_flow_token_ids_utf8_bytes(u, o, 1, -1, v, 0, c, sp, ids, 64, r, LATOK_OUT_INT32);\n"
                   "    return rc + latok_vocab_destroy(v);\n}\n")
    strict = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c"]
    subprocess.check_call(strict + [str(src), "-o", str(tmp_path / "use.o")])
    subprocess.check_call(strict + [os.path.join(ROOT, "examples", "token_ids_utf8.c"), "-o", str(tmp_path / "example.o")])


# ---- vocab_table.h on the host ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    """the stand-alone program, built by plain g++ and once more with -fsanitize=address,undefined; it is run directly"""
    exe = tmp_path_factory.mktemp("vocab_" + request.param) / "vocab_harness"
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "vocab_harness.cpp"), "-o", str(exe)])

    def run(script, poison=0xA5):
        out = subprocess.run([str(exe)], input="%02x\n" % poison + script, capture_output=True, text=True)
        assert out.returncode == 0, ({2: "a text load left the buffer", 3: "a table load left the table"}.get(out.returncode, out.returncode),
                                     out.stderr[-2000:])
        return out.stdout.splitlines()

    return run


def _vocab_lines(words, seed, ids=None):
    lines = ["V %x %d" % (seed, len(words))]
    for i, w in enumerate(words):
        lines.append("%s %s" % ("-" if ids is None else ids[i], w.hex() or "-"))
    return lines


def _dict(words, ids=None):
    d = {}
    for i, w in enumerate(words):
        if w:
            d.setdefault(w, i if ids is None else ids[i])
    return d


def _run(harness, words, seed, probes, ids=None, unk=UNK, forms="lw", pads=range(16), damaged=False):
    """probes: tokens -> [(id, slot loads)] per (token, pad, form), checked against the dict; returns (info, loads)"""
    d = _dict(words, ids)
    cases = [(f, pad, t) for t in probes for pad in pads for f in forms]
    script = "\n".join(_vocab_lines(words, seed, ids) + (["F"] if damaged else []) + ["%s %d %d %s" % (f, pad, unk, t.hex()) for f, pad, t in cases]) + "\n"
    loads = None
    for poison in (0x00, 0xFF, 0xA5):      # what surrounds the token in its dwords must not reach the compare
        out = harness(script, poison)
        m = re.match(r"slots (\d+) used (\d+) blob (\d+)$", out[0])
        assert m and len(out) == 1 + len(cases), out[:3]
        n_slots, used = int(m.group(1)), int(m.group(2))
        assert n_slots >= 64 and n_slots >= 2 * len(words) and n_slots & (n_slots - 1) == 0 and n_slots < max(128, 4 * len(words) + 1)
        assert used == len(d), (used, len(d))
        got = [tuple(map(int, line.split())) for line in out[1:]]
        want = [unk if damaged else d.get(t, unk) for _, _, t in cases]
        bad = [(c[0], c[1], len(c[2]), c[2][:24], g[0], w) for c, g, w in zip(cases, got, want) if g[0] != w]
        assert not bad, (poison, bad[:5])
        assert all(1 <= g[1] <= n_slots for g in got)
        loads = [g[1] for g in got]
    return n_slots, loads


def _token(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def _lengths():
    T = hash_wave_bytes()
    return list(range(1, 81)) + list(range(T - 3, T + 4))


def test_a_hit_and_a_miss(harness):
    words = [b"the", b"quick", b"brown", b"fox"]
    _run(harness, words, 0, words + [b"dog", b"th", b"thee", b"quicK", b"Quick", b"f"])
    _run(harness, words, 0x9747B28C, words + [b"dog"], ids=[7, -3, 7, 0x7FFFFFFF], unk=-0x80000000)


def test_every_length_hits_and_its_neighbours_miss(harness):
    rng = random.Random(60)
    words = [_token(rng, n) for n in _lengths()]
    near = []
    for w in words:
        near.append(w[:-1] + bytes([w[-1] ^ 0x01]))          # the last byte differs
        near.append(bytes([w[0] ^ 0x80]) + w[1:])             # the first byte differs
        near.append(w + b"\x00")                              # the blob's zero padding is no byte of the word
        if len(w) > 1:
            near.append(w[:-1])
    for seed in SEEDS:
        _run(harness, words, seed, words + near, pads=(0, 1, 2, 3, 7, 13) if seed else range(16))


def test_duplicates_first_wins_and_the_empty_word_never_matches(harness):
    words = [b"a", b"b", b"a", b"", b"c", b"b", b"", b"a"]
    _run(harness, words, 1, [b"a", b"b", b"c", b"d", b"\x00", b" "], pads=(0, 5))
    _run(harness, words, 1, [b"a", b"b", b"c", b"d"], ids=[10, 11, 12, 13, 14, 15, 16, 17], pads=(0, 5))
    _run(harness, [b"", b""], 0, [b"a", b"\x00"], pads=(0, 3))


@pytest.mark.parametrize("v", [0, 1, 32, 33])
def test_small_vocabularies(harness, v):
    rng = random.Random(v)
    words = [b"w%d" % i + _token(rng, i % 7) for i in range(v)]
    n_slots, _ = _run(harness, words, 5, words + [b"w", b"w33", b"zz"], pads=(0, 1, 6))
    assert n_slots == (64 if v <= 32 else 128)


def _home(word, seed, n_slots):
    return murmur3_ref(word, seed) & (n_slots - 1)


def wrapped_cluster(seed, n_slots, n=20, start=0):
    """n words whose home slot is the LAST slot of an n_slots table, and one more such word that stays outside"""
    found, i = [], start
    while len(found) < n + 1:
        w = b"k%d" % i
        if _home(w, seed, n_slots) == n_slots - 1:
            found.append(w)
        i += 1
    return found[:n], found[n]


def test_a_cluster_at_the_last_slot_wraps(harness):
    seed = 3
    cluster, outsider = wrapped_cluster(seed, 128)
    filler, i = [], 0
    while len(filler) < 20:                                   # 40 words: a 128-slot table; the filler lives far from the wrap
        w = b"f%d" % i
        if 40 <= _home(w, seed, 128) < 100:
            filler.append(w)
        i += 1
    words = cluster + filler
    n_slots, loads = _run(harness, words, seed, cluster + [outsider], forms="l", pads=(0,))
    assert n_slots == 128
    assert loads[:20] == list(range(1, 21)), loads            # the k-th word of the cluster sits k slots behind slot 127: 127, 0, 1, ..
    assert loads[20] == 21                                    # the outsider walks the whole cluster to its empty slot


@pytest.mark.parametrize("seed", SEEDS)
def test_crafted_collisions_are_told_apart_by_their_bytes(harness, seed):
    rng = random.Random(seed)
    T = hash_wave_bytes()
    pairs = []
    for n in (5, 6, 7, 8, 9, 11, 12, 13, 16, 17, 23, 24, 31, 64, 65, 80, T - 1, T, T + 1, T + 2, 600):
        a = bytes(rng.randrange(0x21, 0x7F) for _ in range(n))
        where = mc.positions(n)
        if len(where) > 8:                                    # long strings: both ends, the middle, the tail
            where = where[:2] + [where[len(where) // 2]] + where[-3:]
        pairs += [(a, mc.collide(a, seed, w)) for w in where]
    if seed == 0:
        pairs += list(mc.KNOWN_WORD_PAIRS) + mc.word_pairs(0)
    assert len(pairs) > 60 and all(murmur3_ref(a, seed) == murmur3_ref(b, seed) and a != b and len(a) == len(b) for a, b in pairs)
    only_a = [a for a, _ in pairs]
    _run(harness, only_a, seed, [b for _, b in pairs] + only_a, pads=(0, 1, 2, 3))          # every b is unknown
    both = [w for p in pairs for w in p]
    _run(harness, both, seed, both, pads=(0, 3))                                            # each its own id
    _run(harness, both[::-1], seed, both, ids=list(range(100, 100 + len(both))), pads=(2,))


def test_a_table_without_an_empty_slot_ends_the_probe(harness):
    words = [b"w%d" % i for i in range(40)]
    n_slots, loads = _run(harness, words, 0, words[:5] + [b"other"], damaged=True, unk=-5, pads=(0, 7))
    assert set(loads) == {n_slots}                            # every probe gave up after exactly n_slots steps


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_vocab_create_refuses_bad_arguments_before_it_asks_for_a_device():
    code = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import _lib
lib = _lib.load()
words = np.frombuffer(b"abcde", np.uint8)
h = C.c_void_p()
def create(off, n, out=h, w=words):
    off = np.array(off, np.int64)
    return lib.latok_vocab_create(w.ctypes.data if w is not None else None, off.ctypes.data, n, None, 0, C.byref(out) if out is not None else None)
for off, n, needle in (([1, 2, 5], 2, "start at 0"), ([0, 3, 2], 2, "non-decreasing"), ([0, -1, 5], 2, "non-decreasing"),
                       ([0, 2, 5], -1, "n_words"), ([0, 2, 5], 1 << 31, "n_words"), ([0, 1 << 32], 1, "2^32")):
    rc = create(off, n)
    assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), (off, n, rc, _lib.last_error())
    assert not h.value
assert lib.latok_vocab_create(words.ctypes.data, None, 1, None, 0, C.byref(h)) == _lib.ERR_INVALID and "word_off" in _lib.last_error()
assert create([0, 2, 5], 2, out=None) == _lib.ERR_INVALID and "vocab_out" in _lib.last_error()
assert create([0, 2, 5], 2, w=None) == _lib.ERR_INVALID and "words" in _lib.last_error()
assert lib.latok_vocab_info(None, None, None, None, None) == _lib.ERR_INVALID
assert lib.latok_vocab_destroy(None) == 0
# good arguments get as far as the device, and none was initialised
assert create([0, 2, 5], 2) == _lib.ERR_NOT_INIT and not h.value
# the ids calls: a stray flag bit first, then the missing device; nothing is written
u8, boff = np.frombuffer(b"abc def", np.uint8), np.array([0, 7], np.int64)
ids, cnt, n, res = np.full(8, 0x5A5A5A5A, np.int32), np.full(1, -7, np.int64), C.c_int64(0), np.zeros(2, np.int64)
for flags in (4, 64, 1 << 20):
    rc = lib.latok_token_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, None, -1, cnt.ctypes.data, None, ids.ctypes.data, 8, C.byref(n), flags, None)
    assert rc == _lib.ERR_INVALID and "flag" in _lib.last_error(), rc
    rc = lib.latok_flow_token_ids_utf8_bytes(u8.ctypes.data, boff.ctypes.data, 1, 7, None, -1, cnt.ctypes.data, None, ids.ctypes.data, 8, res.ctypes.data, flags)
    assert rc == _lib.ERR_INVALID and "flag" in _lib.last_error(), rc
rc = lib.latok_token_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, None, -1, cnt.ctypes.data, None, ids.ctypes.data, 8, C.byref(n), 0, None)
assert rc == _lib.ERR_NOT_INIT, rc
rc = lib.latok_flow_token_ids_utf8_bytes(u8.ctypes.data, boff.ctypes.data, 1, 7, None, -1, cnt.ctypes.data, None, ids.ctypes.data, 8, res.ctypes.data, 0)
assert rc == _lib.ERR_NOT_INIT, rc
assert (ids == 0x5A5A5A5A).all() and cnt[0] == -7
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_a_bad_unk_id_is_a_value_error_before_any_device():
    """LATOK_DEVICE names a device no machine has: anything that reached the library's init would raise RuntimeError instead"""
    code = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import batch
u8, boff = np.frombuffer(b"abc def", np.uint8), np.array([0, 7], np.int64)
fake = batch.Vocab.__new__(batch.Vocab)          # no device, so no real vocabulary: unk_id is looked at first
fake.handle = None
for unk in (1 << 31, -(1 << 31) - 1, 1 << 40, 1.5, "0", None, True, b"\x00"):
    for call in (lambda: batch.token_ids_utf8_csr(u8, boff, fake, unk), lambda: batch.token_ids_utf8_batch([b"abc def"], fake, unk),
                 lambda: batch.token_ids_batch(["abc def"], fake, unk_id=unk), lambda: batch.token_ids_utf8_batch([], fake, unk),
                 lambda: batch.flow_token_ids_utf8_bytes(0x1000, 0x2000, 1, 7, fake, None, None, 0x3000, 7, 0x5000, unk_id=unk)):
        try:
            call()
        except ValueError as e:
            assert "unk_id" in str(e), e
            continue
        raise SystemExit("no ValueError for unk_id=%%r" %% (unk,))
for bad_vocab in (fake, None, {"a": 1}):
    try:
        batch.token_ids_utf8_csr(u8, boff, bad_vocab)
        raise SystemExit("no ValueError for the vocabulary")
    except ValueError as e:
        assert "vocab" in str(e)
for kw in (dict(seed=-1), dict(seed=1 << 32), dict(ids=[1]), dict(ids=[1 << 31, 0]), dict(ids=[0.5, 1.0])):
    try:
        batch.Vocab([b"a", "b"], **kw)
        raise SystemExit("no ValueError for %%r" %% (kw,))
    except ValueError:
        pass
# good arguments get as far as the device, and there is none: RuntimeError, no CPU fallback
try:
    batch.Vocab([b"a", "b"], ids=[5, -5], seed=7)
    raise SystemExit("no RuntimeError")
except RuntimeError:
    pass
print("ok")
""" % ROOT
    env = dict(os.environ, LATOK_DEVICE="4095")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


# ---- the flow's ranges -----------------------------------------------------------------------------------------------------
def _ranges(utf8, byte_off, counts, spans, ids, result, n_str, total_bytes, cap, flags=0):
    from latok_amd import _lib
    fn = _lib.load().latok_debug_flow_ids_ranges
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    addr = np.array([utf8, byte_off, counts, spans, ids, result], np.uint64)
    lo, nb, wr = np.zeros(16, np.uint64), np.zeros(16, np.uint64), np.zeros(16, np.int32)
    n = fn(addr.ctypes.data, n_str, total_bytes, cap, flags, lo.ctypes.data, nb.ctypes.data, wr.ctypes.data, 16)
    assert n > 0
    return [(int(lo[i]), int(nb[i]), "w" if wr[i] else "r") for i in range(n)]


A = dict(utf8=0x1000000, byte_off=0x2000000, counts=0x3000000, spans=0x4000000, ids=0x5000000, result=0x6000000)
N_STR, BYTES = 1000, 300000


def test_the_ranges_an_id_batch_notes():
    for flags, rec in ((0, 8), (2, 4)):
        r = _ranges(**A, n_str=N_STR, total_bytes=BYTES, cap=5000, flags=flags)
        assert sorted(r) == sorted([(A["result"], 16, "w"), (A["ids"], 5000 * 4, "w"), (A["spans"], 5000 * 2 * rec, "w"),
                                    (A["counts"], N_STR * rec, "w"), (A["utf8"], BYTES, "r"), (A["byte_off"], (N_STR + 1) * 8, "r")])
        # the only bound: one token per byte, whatever the capacity says
        for cap in (BYTES, BYTES + 1, 1 << 40, 1 << 62, (1 << 63) - 1):
            r = _ranges(**A, n_str=N_STR, total_bytes=BYTES, cap=cap, flags=flags)
            assert (A["ids"], BYTES * 4, "w") in r and (A["spans"], BYTES * 2 * rec, "w") in r and len(r) == 6, cap
    r = _ranges(**dict(A, counts=0, spans=0), n_str=N_STR, total_bytes=BYTES, cap=5000)   # not asked for: nothing tracked for them
    assert all(nb == 0 for lo, nb, _ in r if lo == 0)


def test_a_second_id_batch_on_the_same_id_buffer_is_ordered_behind_the_first():
    from latok_amd import _lib
    fn = _lib.load().latok_debug_flow_route
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]

    def submit(ranges):
        lo = np.array([r[0] for r in ranges], np.uint64)
        nb = np.array([r[1] for r in ranges], np.uint64)
        wr = np.array([r[2] == "w" for r in ranges], np.int32)
        d = C.c_int(0)
        s = fn(2, lo.ctypes.data, nb.ctypes.data, wr.ctypes.data, len(ranges), C.byref(d))
        assert s >= 0
        return s, d.value

    B = {k: v + 0x80000000 for k, v in A.items()}
    for shared, want in ((None, (1, 0)), ("ids", (0, 0)), ("ids_tail", (0, 0))):
        fn(2, None, None, None, -1, None)
        b = dict(B)
        if shared == "ids":
            b["ids"] = A["ids"]
        elif shared == "ids_tail":
            b["ids"] = A["ids"] + 4 * (5000 - 1)
        assert submit(_ranges(**A, n_str=N_STR, total_bytes=BYTES, cap=5000)) == (0, 0)
        assert submit(_ranges(**b, n_str=N_STR, total_bytes=BYTES, cap=5000)) == want, shared
        fn(2, None, None, None, -1, None)
