"""featurize of UTF-8 in byte space (include/latok_hip.h: latok_token_features_utf8_bytes_batch, latok_flow_token_features_utf8_bytes),
the parts that need no device: the two entry points exist in the library, the header and latok_amd/_lib.py with one arity; the
Python wrappers check their arguments before they touch the library; the C entry refuses a NULL feature buffer; nothing is
computed without a device; and the memory ranges a flow batch of the new form notes -- four result words, counts, the 4-field
records, the feature sums, the inputs -- make the flow's router order a second batch behind the first whenever they share one,
also when a caller passes a huge "unbounded" capacity (the tracked length is clamped to what the batch can write)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKING, FLOW = "latok_token_features_utf8_bytes_batch", "latok_flow_token_features_utf8_bytes"
BYTES_FEATS = 4   # api.cpp: kU8BytesFeats
OUT_INT32 = 2


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
    for name, n_args in ((BLOCKING, 11), (FLOW, 10)):
        assert name in exported, name
        args = _header_decl(name)
        res, bound = _lib.SIGNATURES[name]
        assert res is C.c_int and len(bound) == len(args) == n_args, (name, len(bound), len(args))
        for a, b in zip(args, bound):
            if a.startswith("int64_t* n_tokens_out"):
                assert b is C.POINTER(C.c_int64)
                continue
            want = C.c_void_p if "*" in a else (C.c_int64 if a.startswith("int64_t") else C.c_int)
            assert b is want, (name, a, b)
        assert getattr(lib, name).argtypes == bound
    # the same argument list as the code-point forms they stand beside
    assert _lib.SIGNATURES[BLOCKING] == _lib.SIGNATURES["latok_token_features_utf8_batch"]
    assert _lib.SIGNATURES[FLOW] == _lib.SIGNATURES["latok_flow_token_features_utf8"]
    for name in ("token_features_utf8_bytes_csr", "featurize_utf8_bytes_batch", "flow_token_features_utf8_bytes"):
        assert callable(getattr(batch, name)), name


def test_header_with_the_new_calls_is_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "latok_hip.h"\n'
                   "int f(const uint8_t* u, const int64_t* o, int64_t* c, int64_t* s, int8_t* f8, int64_t* n, int64_t* r) {\n"
                   "    return latok_token_features_utf8_bytes_batch(u, o, 1, -1, c, s, f8, 8, n, LATOK_OUT_INT32, NULL) +\n"
                   "           latok_flow_token_features_utf8_bytes(u, o, 1, -1, c, s, f8, 8, r, 0);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


def test_python_argument_checks_need_no_device():
    from latok_amd import batch
    u8 = np.frombuffer(b"abc def", np.uint8)
    for bad_off in (np.zeros((2, 2), np.int64), np.zeros(0, np.int64), np.array([0, 3, 99], np.int64)):
        with pytest.raises(ValueError, match="byte_off"):
            batch.token_features_utf8_bytes_csr(u8, bad_off)
    with pytest.raises(ValueError, match="dtype"):
        batch.token_features_utf8_bytes_csr(u8, np.array([0, 7], np.int64), dtype=np.int16)
    assert batch.featurize_utf8_bytes_batch([]) == []


def test_c_entry_refuses_a_null_feature_buffer():
    from latok_amd import _lib
    lib = _lib.load()
    u8 = np.frombuffer(b"abc def", np.uint8)
    boff = np.array([0, 7], np.int64)
    counts, spans, n = np.zeros(1, np.int64), np.zeros((7, 4), np.int64), C.c_int64(5)
    rc = lib.latok_token_features_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, counts.ctypes.data, spans.ctypes.data, None, 7,
                                                   C.byref(n), 0, None)
    assert rc == _lib.ERR_INVALID and "features_out" in _lib.last_error()
    assert not spans.any()


def test_nothing_is_computed_without_a_device():
    """a fresh interpreter that never initialises a context: the C entries answer LATOK_ERR_NOT_INIT; the Python wrappers, told to
    use a device that does not exist, raise RuntimeError -- there is no CPU fallback to fall into"""
    code = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from latok_amd import _lib, batch
lib = _lib.load()
u8 = np.frombuffer(b"abc def", np.uint8)
boff = np.array([0, 7], np.int64)
counts, spans, feats, n = np.zeros(1, np.int64), np.zeros((7, 4), np.int64), np.zeros((7, 25), np.int8), C.c_int64(0)
rc = lib.latok_token_features_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 1, 7, counts.ctypes.data, spans.ctypes.data,
                                               feats.ctypes.data, 7, C.byref(n), 0, None)
assert rc == _lib.ERR_NOT_INIT, rc
res = np.zeros(4, np.int64)
rc = lib.latok_flow_token_features_utf8_bytes(u8.ctypes.data, boff.ctypes.data, 1, 7, counts.ctypes.data, spans.ctypes.data,
                                              feats.ctypes.data, 7, res.ctypes.data, 0)
assert rc == _lib.ERR_NOT_INIT, rc
assert not spans.any() and not feats.any()
for call in (lambda: batch.token_features_utf8_bytes_csr(u8, boff), lambda: batch.featurize_utf8_bytes_batch([b"abc def"]),
             lambda: batch.flow_token_features_utf8_bytes(0x1000, 0x2000, 1, 7, 0x3000, 0x4000, 0x5000, 7, 0x6000)):
    try:
        call()
    except RuntimeError:
        continue
    raise SystemExit("no RuntimeError")
print("ok")
""" % ROOT
    env = dict(os.environ, LATOK_DEVICE="4095")   # (no machine has that many devices: latok_init fails with or without a GPU)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def _ranges(what, utf8, byte_off, a2, a3, feat, result, n_str, total_bytes, cap, flags=0):
    """the range list a UTF-8 flow batch notes (api.cpp: latok_debug_flow_utf8_ranges) as [(lo, bytes, 'w' | 'r')]"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_flow_utf8_ranges
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    addr = np.array([utf8, byte_off, a2, a3, feat, result, 0, 0], np.uint64)
    lo, nb, wr = np.zeros(16, np.uint64), np.zeros(16, np.uint64), np.zeros(16, np.int32)
    n = fn(what, addr.ctypes.data, n_str, total_bytes, cap, flags, lo.ctypes.data, nb.ctypes.data, wr.ctypes.data, 16)
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


A = dict(utf8=0x1000000, byte_off=0x2000000, a2=0x3000000, a3=0x4000000, feat=0x5000000, result=0x6000000)
B = {k: v + 0x80000000 for k, v in A.items()}
N_STR, BYTES = 1000, 300000


def test_the_ranges_a_byte_space_featurize_batch_notes():
    for flags, rec in ((0, 8), (OUT_INT32, 4)):
        r = _ranges(BYTES_FEATS, **A, n_str=N_STR, total_bytes=BYTES, cap=5000, flags=flags)
        assert sorted(r) == sorted([(A["result"], 32, "w"), (A["a2"], N_STR * rec, "w"), (A["a3"], 5000 * 4 * rec, "w"),
                                    (A["feat"], 5000 * 25, "w"), (A["utf8"], BYTES, "r"), (A["byte_off"], (N_STR + 1) * 8, "r")])
        # a capacity beyond one token per byte -- up to sizes whose byte count would wrap -- is tracked as what can be written
        for cap in (BYTES, BYTES + 1, 1 << 40, 1 << 60, (1 << 63) - 1):
            r = _ranges(BYTES_FEATS, **A, n_str=N_STR, total_bytes=BYTES, cap=cap, flags=flags)
            assert (A["a3"], BYTES * 4 * rec, "w") in r and (A["feat"], BYTES * 25, "w") in r and len(r) == 6, cap
    # an empty batch still clears its result words and counts on a slot's stream; no record range
    r = _ranges(BYTES_FEATS, **A, n_str=N_STR, total_bytes=0, cap=5000)
    assert (A["result"], 32, "w") in r and (A["a2"], N_STR * 8, "w") in r
    assert all(nb == 0 for lo, nb, _ in r if lo in (A["a3"], A["feat"], A["utf8"]))


@pytest.mark.parametrize("cap", [5000, 1 << 62])
@pytest.mark.parametrize("shared", ["result", "records", "counts", "feat", "feat_tail", "utf8_written", None])
def test_a_second_batch_that_shares_one_buffer_is_ordered_behind_the_first(shared, cap):
    """turn order would put the second batch on slot 1; sharing only the last result word, the records, the counts, the feature
    sums (or their last byte), or writing into the first one's input sends it to slot 0, behind the first -- with a sane capacity
    and with one whose byte size would overflow"""
    submit, reset = _router()
    n_rec = min(cap, BYTES)
    first = _ranges(BYTES_FEATS, **A, n_str=N_STR, total_bytes=BYTES, cap=cap)
    b = dict(B)
    if shared == "result":
        b["result"] = A["result"] + 24
    elif shared == "records":
        b["a3"] = A["a3"]
    elif shared == "counts":
        b["a2"] = A["a2"]
    elif shared == "feat":
        b["feat"] = A["feat"]
    elif shared == "feat_tail":
        b["feat"] = A["feat"] + n_rec * 25 - 1      # the last byte the first batch's sums can reach
    elif shared == "utf8_written":
        b["a3"] = A["utf8"] + 64
    second = _ranges(BYTES_FEATS, **b, n_str=N_STR, total_bytes=BYTES, cap=cap)
    assert submit(first) == (0, 0)
    assert submit(second) == ((1, 0) if shared is None else (0, 0))
    reset()
    # an unrelated code-point batch on the other slot in between changes nothing
    assert submit(first) == (0, 0)
    assert submit(_ranges(3, **{k: v + 0x40000000 for k, v in A.items()}, n_str=N_STR, total_bytes=BYTES, cap=5000)) == (1, 0)
    assert submit(second) == (0, 0)
    reset()
