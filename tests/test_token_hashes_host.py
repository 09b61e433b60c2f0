"""Token hashes (include/latok_hip.h: latok_token_hashes_utf8_bytes_batch, latok_flow_token_hashes_utf8_bytes), the parts that need
no device: the two entry points exist in the library, the header and latok_amd/_lib.py with one arity; the header stays C99 and the
example compiles; the two host implementations of MurmurHash3 x86_32 give the published vectors and agree; token_hash.h, compiled
by g++, gives the same words in its lane form and in its wave form, inside a poisoned buffer that ends with the token's last dword;
the Python wrappers refuse a bad seed before they touch the library; nothing is computed without a device; and the ranges a flow
batch notes keep a second batch ordered behind the first, also under an "unbounded" capacity."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers.murmur3_ref import SEEDS, VECTORS, murmur3_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKING, FLOW = "latok_token_hashes_utf8_bytes_batch", "latok_flow_token_hashes_utf8_bytes"


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


def test_entry_points_are_exported_declared_and_bound():
    from latok_amd import _lib, batch
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "latok_amd", "liblatok_hip.so")], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name, n_args in ((BLOCKING, 12), (FLOW, 11)):
        assert name in exported, name
        args = _header_decl(name)
        res, bound = _lib.SIGNATURES[name]
        assert res is C.c_int and len(bound) == len(args) == n_args, (name, len(bound), len(args))
        for a, b in zip(args, bound):
            if a.startswith("int64_t* n_tokens_out"):
                assert b is C.POINTER(C.c_int64)
                continue
            if a == "uint32_t seed":
                assert b is C.c_uint32
                continue
            want = C.c_void_p if "*" in a else (C.c_int64 if a.startswith("int64_t") else C.c_int)
            assert b is want, (name, a, b)
        assert sum(a == "uint32_t seed" for a in args) == 1
        assert getattr(lib, name).argtypes == bound
    for name in ("token_hashes_utf8_csr", "token_hashes_utf8_batch", "token_hashes_batch", "flow_token_hashes_utf8_bytes", "murmur3_32"):
        assert callable(getattr(batch, name)), name
    # the header comment carries the definition, names the function and cites the reference
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    for name in (BLOCKING, FLOW):
        comment = text[:text.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert "default_tokenizer.py:149-160" in comment and "MurmurHash3 x86_32" in comment, name
    comment = text[:text.index("int %s(" % BLOCKING)].rsplit("/*", 1)[1]
    assert "murmurhash3_32" in comment and "int32" in comment and "positive=True" in comment
    assert "latok_token_spans_utf8_bytes_batch" in comment and "hashes_out[rank(s, k)]" in comment
    assert hash_wave_bytes() >= 64


def test_header_with_the_new_calls_is_c99_and_the_example_compiles(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "latok_hip.h"\n'
                   "int f(const uint8_t* u, const int64_t* o, int64_t* c, int64_t* sp, uint32_t* h, int64_t* n, int64_t* r) {\n"
                   "    return latok_token_hashes_utf8_bytes_batch(u, o, 1, -1, 0x9747b28cu, c, sp, h, 64, n, 0, NULL) +\n"
                   "           latok_token_hashes_utf8_bytes_batch(u, o, 1, -1, 0u, NULL, NULL, h, 64, n, LATOK_OUT_INT32, NULL) +\n"
                   "           latok_flow_token_hashes_utf8_bytes(u, o, 1, -1, 1u, c, sp, h, 64, r, LATOK_OUT_INT32);\n}\n")
    strict = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c"]
    subprocess.check_call(strict + [str(src), "-o", str(tmp_path / "use.o")])
    subprocess.check_call(strict + [os.path.join(ROOT, "examples", "token_hashes_utf8.c"), "-o", str(tmp_path / "example.o")])


# ---- the two host implementations ------------------------------------------------------------------------------------------
def _random_byte_strings(n, hi, seed):
    rng = random.Random(seed)
    return [bytes(rng.getrandbits(8) for _ in range(rng.randint(0, hi))) for _ in range(n)]


def test_both_host_implementations_give_the_published_vectors_and_agree():
    from latok_amd import batch
    for data, seed, want in VECTORS:
        assert murmur3_ref(data, seed) == want, (data, seed, hex(murmur3_ref(data, seed)))
        assert batch.murmur3_32(data, seed) == want, (data, seed, hex(batch.murmur3_32(data, seed)))
    rng = random.Random(8)
    for data in _random_byte_strings(2000, 300, 1):
        seed = rng.choice(SEEDS + (rng.getrandbits(32),))
        assert batch.murmur3_32(data, seed) == murmur3_ref(data, seed), (data, seed)
    assert batch.murmur3_32(bytearray(b"test")) == batch.murmur3_32(memoryview(b"test")) == 0xBA6BD213
    assert batch.murmur3_32(b"test", np.uint32(0x9747B28C)) == 0x704B81DC


def test_scikit_learn_agrees_where_it_is_installed():
    sk = pytest.importorskip("sklearn.utils")
    for data, seed, want in VECTORS:
        assert sk.murmurhash3_32(data, seed, positive=True) == want
        assert sk.murmurhash3_32(data, seed) & 0xFFFFFFFF == want                  # the same word read as int32
    for data in _random_byte_strings(300, 300, 2):
        assert sk.murmurhash3_32(data, 7, positive=True) == murmur3_ref(data, 7)


# ---- token_hash.h on the host ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("token_hash") / "token_hash_harness"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "token_hash_harness.cpp"), "-o", str(exe)])

    def run(cases, poison):
        """cases: (form, pad, seed, token bytes) -> the hashes; the harness exits with 2 when a load left the buffer"""
        text = "%02x\n" % poison + "".join("%s %d %x %s\n" % (f, pad, seed, data.hex() or "-") for f, pad, seed, data in cases)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert out.returncode == 0, ("a load outside the buffer" if out.returncode == 2 else out.stderr)
        got = [int(v, 16) for v in out.stdout.split()]
        assert len(got) == len(cases)
        return got

    return run


def _token(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def _check_cases(harness, cases):
    want = [murmur3_ref(data, seed) for _, _, seed, data in cases]
    for poison in (0x00, 0xFF, 0xA5):      # what surrounds the token in its dwords must not reach the hash
        got = harness(cases, poison)
        bad = [(c[0], c[1], hex(c[2]), len(c[3]), hex(g), hex(w)) for c, g, w in zip(cases, got, want) if g != w]
        assert not bad, (poison, bad[:5])


def test_lane_form_every_length_at_every_alignment(harness):
    rng = random.Random(40)
    cases = [("l", pad, SEEDS[(n + pad) % 4], _token(rng, n)) for n in range(0, 81) for pad in range(16)]
    cases += [("l", pad, seed, data) for data, seed, _ in VECTORS for pad in (0, 1, 2, 3, 13)]
    _check_cases(harness, cases)
    assert harness([("l", 0, s, d) for d, s, _ in VECTORS], 0x5A) == [w for _, _, w in VECTORS]


def test_wave_form_around_every_round_and_at_the_threshold(harness):
    rng = random.Random(41)
    T = hash_wave_bytes()
    lengths = sorted({m * 256 + d for m in range(1, 9) for d in range(-3, 4)} | {T - 1, T, T + 1} | {1, 3, 4, 5, 255, 257, 1000, 5000})
    cases = [("w", pad, SEEDS[(n + pad) % 4], _token(rng, n)) for n in lengths for pad in (0, 1, 2, 3, 7, 14)]
    cases += [("w", pad, seed, data) for data, seed, _ in VECTORS for pad in (0, 3)]
    # the two forms meet at the threshold: the same token through both
    cases += [(f, 5, 1, _token(random.Random(n), n)) for n in (T - 1, T, T + 1) for f in "lw"]
    _check_cases(harness, cases)


# ---- Python argument checks ------------------------------------------------------------------------------------------------
def test_a_bad_seed_is_a_value_error_before_any_device():
    """LATOK_DEVICE names a device no machine has: anything that reached the library's init would raise RuntimeError instead"""
    code = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import batch
u8, boff = np.frombuffer(b"abc def", np.uint8), np.array([0, 7], np.int64)
for seed in (-1, 1 << 32, 1 << 40, 1.5, "0", None, True, b"\x00"):
    for call in (lambda: batch.token_hashes_utf8_csr(u8, boff, seed), lambda: batch.token_hashes_utf8_batch([b"abc def"], seed),
                 lambda: batch.token_hashes_batch(["abc def"], seed=seed), lambda: batch.murmur3_32(b"abc", seed),
                 lambda: batch.token_hashes_utf8_batch([], seed),
                 lambda: batch.flow_token_hashes_utf8_bytes(0x1000, 0x2000, 1, 7, None, None, 0x3000, 7, 0x5000, seed=seed)):
        try:
            call()
        except ValueError:
            continue
        raise SystemExit("no ValueError for seed=%%r" %% (seed,))
try:
    batch.token_hashes_utf8_csr(u8, boff, 0, dtype=np.int16)
    raise SystemExit("no ValueError for dtype")
except ValueError:
    pass
# a good seed gets as far as the device, and there is none: RuntimeError, no CPU fallback
for call in (lambda: batch.token_hashes_utf8_csr(u8, boff), lambda: batch.token_hashes_utf8_batch([b"abc def"], 0xFFFFFFFF),
             lambda: batch.token_hashes_batch(["abc def"]), lambda: batch.token_hashes_utf8_csr(u8, boff, np.uint32(7), spans=True),
             lambda: batch.flow_token_hashes_utf8_bytes(0x1000, 0x2000, 1, 7, None, None, 0x3000, 7, 0x5000)):
    try:
        call()
    except RuntimeError:
        continue
    raise SystemExit("no RuntimeError")
assert batch.token_hashes_utf8_batch([]) == []
assert batch.murmur3_32(b"test", 0x9747b28c) == 0x704B81DC      # the host function needs no device
print("ok")
""" % ROOT
    env = dict(os.environ, LATOK_DEVICE="4095")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_c_entries_refuse_bad_arguments_and_compute_nothing_without_a_device():
    code = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import _lib
lib = _lib.load()
u8, boff = np.frombuffer(b"abc def", np.uint8), np.array([0, 7], np.int64)
h, cnt, n, res = np.full(8, 0x5A5A5A5A, np.uint32), np.full(1, -7, np.int64), C.c_int64(0), np.zeros(2, np.int64)
for flags in (4, 64, 1 << 20):   # a stray flag bit is refused before anything else, initialised or not
    rc = lib.latok_token_hashes_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, 0, cnt.ctypes.data, None, h.ctypes.data, 8, C.byref(n), flags, None)
    assert rc == _lib.ERR_INVALID and "flag" in _lib.last_error(), rc
    rc = lib.latok_flow_token_hashes_utf8_bytes(u8.ctypes.data, boff.ctypes.data, 1, 7, 0, cnt.ctypes.data, None, h.ctypes.data, 8, res.ctypes.data, flags)
    assert rc == _lib.ERR_INVALID and "flag" in _lib.last_error(), rc
rc = lib.latok_token_hashes_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, 0, cnt.ctypes.data, None, h.ctypes.data, 8, C.byref(n), 0, None)
assert rc == _lib.ERR_NOT_INIT, rc
rc = lib.latok_flow_token_hashes_utf8_bytes(u8.ctypes.data, boff.ctypes.data, 1, 7, 0, cnt.ctypes.data, None, h.ctypes.data, 8, res.ctypes.data, 0)
assert rc == _lib.ERR_NOT_INIT, rc
assert (h == 0x5A5A5A5A).all() and cnt[0] == -7
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


# ---- the flow's routing ----------------------------------------------------------------------------------------------------
def _ranges(utf8, byte_off, counts, spans, hashes, result, n_str, total_bytes, cap, flags=0):
    from latok_amd import _lib
    fn = _lib.load().latok_debug_flow_hashes_ranges
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    addr = np.array([utf8, byte_off, counts, spans, hashes, result], np.uint64)
    lo, nb, wr = np.zeros(16, np.uint64), np.zeros(16, np.uint64), np.zeros(16, np.int32)
    n = fn(addr.ctypes.data, n_str, total_bytes, cap, flags, lo.ctypes.data, nb.ctypes.data, wr.ctypes.data, 16)
    assert n > 0
    return [(int(lo[i]), int(nb[i]), "w" if wr[i] else "r") for i in range(n)]


def _router():
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

    def reset():
        fn(2, None, None, None, -1, None)

    reset()
    return submit, reset


A = dict(utf8=0x1000000, byte_off=0x2000000, counts=0x3000000, spans=0x4000000, hashes=0x5000000, result=0x6000000)
B = {k: v + 0x80000000 for k, v in A.items()}
N_STR, BYTES = 1000, 300000


def test_the_ranges_a_hash_batch_notes():
    for flags, rec in ((0, 8), (2, 4)):
        r = _ranges(**A, n_str=N_STR, total_bytes=BYTES, cap=5000, flags=flags)
        assert sorted(r) == sorted([(A["result"], 16, "w"), (A["hashes"], 5000 * 4, "w"), (A["spans"], 5000 * 2 * rec, "w"),
                                    (A["counts"], N_STR * rec, "w"), (A["utf8"], BYTES, "r"), (A["byte_off"], (N_STR + 1) * 8, "r")])
        # the only bound: one token per byte, whatever the capacity says
        for cap in (BYTES, BYTES + 1, 1 << 40, 1 << 62, (1 << 63) - 1):
            r = _ranges(**A, n_str=N_STR, total_bytes=BYTES, cap=cap, flags=flags)
            assert (A["hashes"], BYTES * 4, "w") in r and (A["spans"], BYTES * 2 * rec, "w") in r and len(r) == 6, cap
    r = _ranges(**dict(A, counts=0, spans=0), n_str=N_STR, total_bytes=BYTES, cap=5000)   # not asked for: nothing tracked for them
    assert all(nb == 0 for lo, nb, _ in r if lo == 0)


@pytest.mark.parametrize("cap", [5000, 1 << 62])
@pytest.mark.parametrize("shared", ["result", "hashes", "hashes_tail", "spans", "spans_tail", "counts", "utf8_written", None])
def test_a_second_hash_batch_on_the_same_buffer_is_ordered_behind_the_first(shared, cap):
    submit, reset = _router()
    n_tok = min(cap, BYTES)
    first = _ranges(**A, n_str=N_STR, total_bytes=BYTES, cap=cap)
    b = dict(B)
    if shared == "result":
        b["result"] = A["result"] + 8
    elif shared == "hashes":
        b["hashes"] = A["hashes"]
    elif shared == "hashes_tail":
        b["hashes"] = A["hashes"] + 4 * (n_tok - 1)        # the last word the first batch can write
    elif shared == "spans":
        b["spans"] = A["spans"]
    elif shared == "spans_tail":
        b["spans"] = A["spans"] + 16 * (n_tok - 1)
    elif shared == "counts":
        b["counts"] = A["counts"]
    elif shared == "utf8_written":
        b["hashes"] = A["utf8"] + 64
    second = _ranges(**b, n_str=N_STR, total_bytes=BYTES, cap=cap)
    assert submit(first) == (0, 0)
    assert submit(second) == ((1, 0) if shared is None else (0, 0))
    reset()
