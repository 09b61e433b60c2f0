"""Token counting (include/latok_hip.h: latok_counter_*, latok_count_tokens_utf8_bytes_batch), the parts that need no device: the
entry points exist in the library, the header and latok_amd/_lib.py with one arity, the header stays C99 and the example compiles;
count_table.h, compiled by g++ as a stand-alone program (plain, with the address and undefined-behaviour sanitizers, and with the
thread sanitizer for the threaded cases), finds and enters tokens of every length at every pair of byte phases inside a poisoned
buffer and gives the counts of a Python Counter -- fresh and resident compares, a word ending at the buffer's last byte, crafted
hash collisions in both orders, a cluster that wraps at the last slot, a full table that ends the probe by its bound, 8 threads
entering overlapping word sets into one table; bad arguments are refused before a device is asked for."""
import collections
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import murmur3_collide as mc
from helpers.murmur3_ref import murmur3_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"latok_counter_create": 4, "latok_counter_destroy": 1, "latok_counter_clear": 1, "latok_counter_info": 7,
           "latok_count_tokens_utf8_bytes_batch": 8, "latok_counter_read": 8}
PROBE_MAX = 128


def limits():
    from latok_amd import _lib
    fn = _lib.load().latok_debug_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(32, np.int64)
    n = fn(out.ctypes.data, 32)
    return n, out


# ---- the surface -----------------------------------------------------------------------------------------------------------
def _header_decl(name):
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    m = re.search(r"^int %s\((.*?)\);" % name, text, re.S | re.M)
    assert m, "%s is not declared in include/latok_hip.h" % name
    args = re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " "))
    return [a.strip() for a in args.split(",")]


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
            if a == "uint32_t seed":
                assert b is C.c_uint32
            elif "*" in a:
                assert b is C.c_void_p or issubclass(b, C._Pointer), (name, a, b)
            else:
                assert b is (C.c_int64 if a.startswith("int64_t") else C.c_int), (name, a, b)
    for name in ("TokenCounter", "count_tokens_utf8_batch"):
        assert callable(getattr(batch, name)), name
    for name in ("update_utf8", "update_utf8_csr", "update", "items", "most_common", "to_vocab", "clear", "close", "__enter__", "__exit__"):
        assert callable(getattr(batch.TokenCounter, name)), name
    assert isinstance(batch.TokenCounter.stats, property)
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    comment = text[:text.index("typedef struct latok_counter")].rsplit("/*", 1)[1]
    for needle in ("tokens    = counted + long + dropped", "no flow form", "FAILED STATE", "2^39", "latok_vocab_create", "lower bound",
                   "latok_token_spans_utf8_bytes_batch", "LATOK_OUT_INT32 included", "serialised by a lock", "unspecified"):
        assert needle in comment, needle


def test_the_limits_gain_the_probe_bound_and_the_accumulator_size():
    n, out = limits()
    assert n == 19
    assert out[14] == 256 and out[17] == PROBE_MAX
    acc = int(out[18])
    assert acc >= 64 and acc & (acc - 1) == 0


def test_header_with_the_new_calls_is_c99_and_the_example_compiles(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "latok_hip.h"\n'
                   "int f(const uint8_t* u, const int64_t* o, uint8_t* w, int64_t* wo, uint64_t* c, int64_t* st) {\n"
                   "    latok_counter* k = NULL;\n"
                   "    int64_t mw, ns, nw, nb; uint32_t seed; int dev, mb;\n"
                   "    int rc = latok_counter_create(1000, 256, 7u, &k) + latok_counter_info(k, &mw, &ns, &mb, &seed, &dev, st);\n"
                   "    rc += latok_count_tokens_utf8_bytes_batch(u, o, 1, -1, k, st, 0, NULL);\n"
                   "    rc += latok_count_tokens_utf8_bytes_batch(u, o, 1, -1, k, NULL, LATOK_DEVICE_PTRS, NULL);\n"
                   "    rc += latok_counter_read(k, NULL, 0, NULL, NULL, 0, &nw, &nb) + latok_counter_read(k, w, nb, wo, c, nw, &nw, &nb);\n"
                   "    return rc + latok_counter_clear(k) + latok_counter_destroy(k);\n}\n")
    strict = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c"]
    subprocess.check_call(strict + [str(src), "-o", str(tmp_path / "use.o")])
    subprocess.check_call(strict + [os.path.join(ROOT, "examples", "count_tokens_utf8.c"), "-o", str(tmp_path / "example.o")])


# ---- count_table.h on the host ---------------------------------------------------------------------------------------------
def _build(tmp_path_factory, kind):
    exe = tmp_path_factory.mktemp("count_" + kind) / "count_table_harness"
    extra = {"plain": [], "sanitized": ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
             "threads": ["-g", "-fsanitize=thread"]}[kind]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread"] + extra + ["-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "count_table_harness.cpp"), "-o", str(exe)])

    def run(script):
        out = subprocess.run([str(exe)], input=script, capture_output=True, text=True)
        assert out.returncode == 0, ({2: "a text load left the buffer", 3: "a blob access left the blob", 4: "a slot stayed fresh"}
                                     .get(out.returncode, out.returncode), out.stderr[-2000:])
        return out.stdout.splitlines()

    return run


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    """the stand-alone program, built by plain g++ and once more with -fsanitize=address,undefined; it is run directly"""
    return _build(tmp_path_factory, request.param)


@pytest.fixture(scope="module")
def harness_tsan(tmp_path_factory):
    """... and with -fsanitize=thread, for the batches that several threads enter"""
    return _build(tmp_path_factory, "threads")


def _table(seed, max_words, probe_max=PROBE_MAX):
    return ["T %x %d %d" % (seed, max_words, probe_max)]


def _batch(tokens, threads=1, poison=0xA5):
    """tokens: [(phase, bytes)]"""
    return ["B %d %02x %d" % (threads, poison, len(tokens))] + ["%d %s" % (p, t.hex()) for p, t in tokens]


def _parse(out, batches):
    """-> n_slots, per batch ([(slot, loads)] or None, counted, dropped, fresh), dump {word: (slot, count)}; a word in two slots fails"""
    it = iter(out)
    n_slots = int(re.match(r"slots (\d+)$", next(it)).group(1))
    res = []
    for n, threads in batches:
        per = [tuple(map(int, next(it).split())) for _ in range(n)] if threads == 1 else None
        m = re.match(r"batch counted (\d+) dropped (\d+) fresh (\d+) blob (\d+)$", next(it))
        res.append((per, int(m.group(1)), int(m.group(2)), int(m.group(3))))
    dump = {}
    for line in it:
        if line == "end":
            break
        slot, word, count = line.split()
        word = bytes.fromhex(word)
        assert word not in dump, ("a word sits in two slots", word)
        dump[word] = (int(slot), int(count))
    return n_slots, res, dump


def _run(harness, seed, max_words, batches, probe_max=PROBE_MAX, threads=1, poisons=(0x00, 0xFF, 0xA5)):
    """enter the batches (lists of (phase, token)) into one table and check the dump against a Counter; returns the last parse"""
    want = collections.Counter(t for b in batches for _, t in b) if threads == 1 else \
        collections.Counter({t: threads * c for t, c in collections.Counter(t for b in batches for _, t in b).items()})
    parsed = None
    for poison in poisons:                  # what surrounds a token in its dwords must not reach a compare or the blob
        script = _table(seed, max_words, probe_max)
        for b in batches:
            script += _batch(b, threads, poison)
        out = harness("\n".join(script + ["D"]) + "\n")
        parsed = _parse(out, [(len(b), threads) for b in batches])
        n_slots, res, dump = parsed
        assert n_slots >= 64 and n_slots >= 2 * max_words and n_slots & (n_slots - 1) == 0
        if all(r[2] == 0 for r in res):     # nothing dropped: exact
            assert {w: c for w, (_, c) in dump.items()} == dict(want), poison
        assert sum(r[1] + r[2] for r in res) == sum(want.values())
    return parsed


def _token(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def test_the_empty_word_is_no_occupied_word(harness):
    assert harness("E\n") == ["ok"]


def test_every_length_at_the_four_phases_of_both_ranges(harness):
    rng = random.Random(61)
    words = [_token(rng, n) for n in range(1, 257)]
    for rep_phase in range(4):
        # first batch: the representative at rep_phase, then the same bytes at all four phases (fresh: text against text), and a
        # near miss of every word (last byte, first byte); second batch: all four phases again (resident: text against the blob)
        first, second = [], []
        for w in words:
            first.append((rep_phase, w))
            first += [(p, w) for p in range(4)]
            first.append(((rep_phase + 1) & 3, w[:-1] + bytes([w[-1] ^ 0x01])))
            first.append(((rep_phase + 2) & 3, bytes([w[0] ^ 0x80]) + w[1:]))
            second += [(p, w) for p in range(4)]
            second.append((rep_phase, w + b"\x00") if len(w) < 256 else (rep_phase, w))      # the blob's padding is no byte of the word
        _, res, dump = _run(harness, 0x9747B28C if rep_phase & 1 else 0, 2048, [first, second], poisons=(0x00, 0xFF) if rep_phase else (0x00, 0xFF, 0xA5))
        assert res[0][2] == res[1][2] == 0
        assert res[0][3] == len({t for _, t in first})
        assert res[1][3] == len({t for _, t in second} - {t for _, t in first})       # the words of the first batch were found resident


def test_a_word_ending_at_the_buffers_last_byte(harness):
    for n in (1, 2, 3, 4, 5, 7, 8, 255, 256):
        for phase in range(4):
            w = bytes(range(1, n + 1)) if n < 255 else bytes((i * 7 + 1) & 0xFF or 1 for i in range(n))
            # the last token ends the text; it equals the first (a compare whose second range ends the buffer) or is new (a claim)
            _run(harness, 5, 16, [[(0, w), (1, b"x"), (phase, w)]], poisons=(0xA5,))
            _run(harness, 5, 16, [[(0, b"y"), (phase, w)], [(phase, w), (0, b"y"), ((phase + 1) & 3, w)]], poisons=(0xA5,))


def test_crafted_collisions_are_told_apart_in_both_orders(harness):
    rng = random.Random(3)
    for seed in (0, 0x9747B28C):
        pairs = []
        for n in (5, 6, 7, 8, 9, 12, 13, 16, 17, 31, 64, 65, 255, 256):
            a = bytes(rng.randrange(0x21, 0x7F) for _ in range(n))
            where = mc.positions(n)
            where = where[:1] + where[-2:] if len(where) > 3 else where
            pairs += [(a, mc.collide(a, seed, w)) for w in where]
        if seed == 0:
            pairs += list(mc.KNOWN_WORD_PAIRS)
        assert len(pairs) > 20 and all(murmur3_ref(a, seed) == murmur3_ref(b, seed) and a != b and len(a) == len(b) for a, b in pairs)
        for order in (lambda a, b: (a, b), lambda a, b: (b, a)):
            both = [(i & 3, w) for i, p in enumerate(pairs) for w in order(*p) * 2] + [(1, pairs[0][0])]
            _, res, dump = _run(harness, seed, 256, [both], poisons=(0xA5,))              # fresh against fresh
            assert all(w in dump for p in pairs for w in p)
            first = [(i & 3, order(*p)[0]) for i, p in enumerate(pairs)]
            second = [((i + 1) & 3, w) for i, p in enumerate(pairs) for w in order(*p)[::-1]]
            _, res, dump = _run(harness, seed, 256, [first, second], poisons=(0xA5,))     # resident first, fresh second
            assert res[0][3] == len({t for _, t in first}) and res[1][3] == len({t for _, t in second} - {t for _, t in first}) > 10
            for a, b in pairs:                                                            # same home slot, neighbouring probes
                assert dump[a][0] != dump[b][0]


def _home(word, seed, n_slots):
    return murmur3_ref(word, seed) & (n_slots - 1)


def test_a_cluster_at_the_last_slot_wraps(harness):
    seed, n_slots = 3, 128
    cluster, i = [], 0
    while len(cluster) < 21:
        w = b"k%d" % i
        if _home(w, seed, n_slots) == n_slots - 1:
            cluster.append(w)
        i += 1
    (_, res, dump) = _run(harness, seed, 64, [[(i & 3, w) for i, w in enumerate(cluster)], [(0, cluster[-1]), (2, cluster[0])]], poisons=(0xA5,))
    per = res[0][0]
    assert [s for s, _ in per] == [(n_slots - 1 + k) % n_slots for k in range(21)]       # 127, 0, 1, ..
    assert [l for _, l in per] == list(range(1, 22))
    assert res[1][0] == [(19, 21), (127, 1)]


def test_a_full_table_ends_the_probe_by_its_bound_and_tallies_dropped(harness):
    words = [b"w%d" % i for i in range(100)]
    for probe_max, bound in ((PROBE_MAX, 64), (16, 16)):
        n_slots, res, dump = _run(harness, 0, 4, [[(i & 3, w) for i, w in enumerate(words)], [(0, w) for w in words]], probe_max=probe_max,
                                  poisons=(0xA5,))
        assert n_slots == 64
        per1, counted1, dropped1, fresh1 = res[0]
        per2, counted2, dropped2, _ = res[1]
        assert dropped1 > 0 and counted1 + dropped1 == 100 and fresh1 == counted1 == len(dump)
        if bound == 64:
            assert fresh1 == 64                                           # the table is full: every slot was reachable
        assert all(l == bound for s, l in per1 + per2 if s == -1)         # a dropped token gave up after exactly `bound` loads
        assert all(l <= bound for _, l in per1 + per2)
        # the second batch finds what is held and drops the rest again: every held count is a lower bound of the true count 2
        assert counted2 == counted1 and dropped2 == dropped1
        assert all(w in set(words) and c == 2 for w, (_, c) in dump.items())


def test_eight_threads_enter_overlapping_word_sets_into_one_table(harness_tsan):
    rng = random.Random(8)
    words = [b"t%d" % i + _token(rng, i % 40) for i in range(300)]
    tokens = [(rng.randrange(4), rng.choice(words)) for _ in range(2000)] + [(i & 3, w) for i, w in enumerate(words)]
    # every thread enters every token, each from another start: the same words are first-claimed by several threads at once
    _, res, dump = _run(harness_tsan, 11, 512, [tokens, tokens[::-1]], threads=8, poisons=(0xA5,))
    assert res[0][2] == res[1][2] == 0 and res[0][3] == 300 and res[1][3] == 0
    assert len(dump) == 300
    # and a table too small for them: no duplicates, the identity, lower bounds
    n_slots, res, dump = _run(harness_tsan, 11, 4, [tokens], threads=8, poisons=(0xA5,))
    true = collections.Counter(t for _, t in tokens)
    assert res[0][2] > 0 and res[0][1] + res[0][2] == 8 * len(tokens) and len(dump) <= n_slots
    assert all(0 < c <= 8 * true[w] for w, (_, c) in dump.items())


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_a_device_is_asked_for():
    code = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import _lib
lib = _lib.load()
h = C.c_void_p()
for mw, mb, needle in ((0, 256, "max_words"), (-1, 256, "max_words"), ((1 << 30) + 1, 256, "max_words"), (10, 0, "max_word_bytes"),
                       (10, 257, "max_word_bytes"), (10, -1, "max_word_bytes"), (10, 1 << 20, "max_word_bytes")):
    rc = lib.latok_counter_create(mw, mb, 0, C.byref(h))
    assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), (mw, mb, rc, _lib.last_error())
    assert not h.value
assert lib.latok_counter_create(10, 256, 0, None) == _lib.ERR_INVALID
# good arguments get as far as the device, and none was initialised
assert lib.latok_counter_create(10, 256, 0, C.byref(h)) == _lib.ERR_NOT_INIT and not h.value
assert lib.latok_counter_create(1 << 30, 1, 0xFFFFFFFF, C.byref(h)) == _lib.ERR_NOT_INIT and not h.value
assert lib.latok_counter_destroy(None) == 0
assert lib.latok_counter_clear(None) == _lib.ERR_INVALID
assert lib.latok_counter_info(None, None, None, None, None, None, None) == _lib.ERR_INVALID
n, nb = C.c_int64(5), C.c_int64(5)
assert lib.latok_counter_read(None, None, 0, None, None, 0, C.byref(n), C.byref(nb)) == _lib.ERR_INVALID
# the update call: a stray flag bit first (LATOK_OUT_INT32 included), then the NULL counter; nothing is written
u8, boff = np.frombuffer(b"abc def", np.uint8), np.array([0, 7], np.int64)
st = np.full(4, -7, np.int64)
for flags in (2, 3, 4, 64, 1 << 20):
    rc = lib.latok_count_tokens_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, None, st.ctypes.data, flags, None)
    assert rc == _lib.ERR_INVALID and "flag" in _lib.last_error(), rc
for flags in (0, 1):
    rc = lib.latok_count_tokens_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, None, st.ctypes.data, flags, None)
    assert rc == _lib.ERR_INVALID and "counter is NULL" in _lib.last_error(), rc
assert (st == -7).all()
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_python_refuses_bad_arguments_with_a_value_error_before_any_device():
    """LATOK_DEVICE names a device no machine has: anything that reached the library's init would raise RuntimeError instead"""
    code = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import batch
for args, kw in (((0,), {}), ((-5,), {}), ((1.5,), {}), (("10",), {}), ((True,), {}), (((1 << 30) + 1,), {}), ((10,), dict(max_word_bytes=0)),
                 ((10,), dict(max_word_bytes=257)), ((10,), dict(max_word_bytes=2.0)), ((10,), dict(seed=-1)), ((10,), dict(seed=1 << 32)),
                 ((10,), dict(seed=None))):
    try:
        batch.TokenCounter(*args, **kw)
    except ValueError:
        continue
    raise SystemExit("no ValueError for %%r %%r" %% (args, kw))
closed = batch.TokenCounter.__new__(batch.TokenCounter)
closed.handle = None
for call in (lambda: closed.update_utf8([b"a b"]), lambda: closed.update(["a b"]), lambda: closed.items(), lambda: closed.clear(),
             lambda: closed.update_utf8_csr(np.frombuffer(b"a b", np.uint8), np.array([0, 3])), lambda: closed.stats, lambda: closed.most_common(3)):
    try:
        call()
    except ValueError as e:
        assert "closed" in str(e), e
        continue
    raise SystemExit("no ValueError for a closed counter")
closed.close()
try:
    batch.count_tokens_utf8_batch([b"a b"], max_words=0)
    raise SystemExit("no ValueError")
except ValueError:
    pass
# good arguments get as far as the device, and there is none: RuntimeError, no CPU fallback
for call in (lambda: batch.TokenCounter(10, max_word_bytes=5, seed=7), lambda: batch.count_tokens_utf8_batch([b"a b"])):
    try:
        call()
        raise SystemExit("no RuntimeError")
    except RuntimeError:
        pass
print("ok")
""" % ROOT
    env = dict(os.environ, LATOK_DEVICE="4095")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)
