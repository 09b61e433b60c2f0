"""UTF-8 in code-point units through the batch flow (include/latok_hip.h: latok_flow_*_utf8), the parts that need no device:
the four entry points exist in the library, the header and latok_amd/_lib.py with one arity, and the memory ranges such a batch
notes -- the 32 bytes of result words, the n_str + 1 code-point row offsets, mask, counts, records, feature sums, inputs -- make
the flow's router (flow_hazards.h) order a second batch behind the first whenever they share any of them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("latok_flow_split_mask_utf8", "latok_flow_split_offsets_utf8", "latok_flow_token_spans_utf8", "latok_flow_token_features_utf8")
MASK, OFFSETS, SPANS, FEATS = range(4)
OUT_INT32 = 2


def _header_decl(name):
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    m = re.search(r"^int %s\((.*?)\);" % name, text, re.S | re.M)
    assert m, "%s is not declared in include/latok_hip.h" % name
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_entry_points_are_exported_declared_and_bound():
    from latok_amd import _lib
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "latok_amd", "liblatok_hip.so")], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert name in exported, name
        args = _header_decl(name)
        res, bound = _lib.SIGNATURES[name]
        assert res is C.c_int and len(bound) == len(args), (name, len(bound), len(args))
        # pointers are bound as void pointers, sizes as int64, flags as int -- position by position
        for a, b in zip(args, bound):
            want = C.c_void_p if "*" in a else (C.c_int64 if a.startswith("int64_t") else C.c_int)
            assert b is want, (name, a, b)
        assert getattr(lib, name).argtypes == bound
    assert len(_header_decl(NAMES[0])) == 8 and len(_header_decl(NAMES[1])) == 9 and len(_header_decl(NAMES[2])) == 9
    assert len(_header_decl(NAMES[3])) == 10
    from latok_amd import batch
    for name in NAMES:
        assert callable(getattr(batch, name[len("latok_"):]))
    import latok
    assert not any(hasattr(latok, name[len("latok_"):]) for name in NAMES)      # the top-level package re-exports nothing new


def test_header_with_the_new_calls_is_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "latok_hip.h"\n'
                   "int f(const uint8_t* u, const int64_t* o, uint64_t* m, int64_t* r, void* c, void* i, int8_t* f8) {\n"
                   "    return latok_flow_split_mask_utf8(u, o, 1, -1, m, 4, r, r) + latok_flow_split_offsets_utf8(u, o, 1, -1, c, i, 8, r, 0) +\n"
                   "           latok_flow_token_spans_utf8(u, o, 1, -1, c, i, 8, r, LATOK_OUT_INT32) +\n"
                   "           latok_flow_token_features_utf8(u, o, 1, -1, c, i, f8, 8, r, 0);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


def _ranges(what, utf8, byte_off, a2, a3, feat, result, n_str, total_bytes, cap, flags=0):
    """the range list a code-point batch notes (api.cpp: latok_debug_flow_utf8_ranges) as [(lo, bytes, 'w' | 'r')]"""
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


# two disjoint sets of buffers, far apart: A and B share nothing unless a test makes them
A = dict(utf8=0x1000000, byte_off=0x2000000, a2=0x3000000, a3=0x4000000, feat=0x5000000, result=0x6000000)
B = {k: v + 0x80000000 for k, v in A.items()}
N_STR, BYTES = 1000, 300000


def test_the_ranges_a_code_point_batch_notes():
    words_b = (BYTES + 63) // 64
    r = _ranges(MASK, **A, n_str=N_STR, total_bytes=BYTES, cap=words_b)
    assert (A["result"], 32, "w") in r                       # four result words
    assert (A["a3"], (N_STR + 1) * 8, "w") in r              # n_str + 1 code-point row offsets
    assert (A["a2"], words_b * 8, "w") in r                  # the mask: ceil(bytes / 64) words always suffice
    assert (A["utf8"], BYTES, "r") in r and (A["byte_off"], (N_STR + 1) * 8, "r") in r and len(r) == 5
    # a smaller mask buffer is noted as it is; a larger one only as far as it can be written
    assert (A["a2"], 80, "w") in _ranges(MASK, **A, n_str=N_STR, total_bytes=BYTES, cap=10)
    assert (A["a2"], words_b * 8, "w") in _ranges(MASK, **A, n_str=N_STR, total_bytes=BYTES, cap=10 * words_b)
    for what, fields in ((OFFSETS, 1), (SPANS, 2), (FEATS, 4)):
        for flags, rec in ((0, 8), (OUT_INT32, 4)):
            r = _ranges(what, **A, n_str=N_STR, total_bytes=BYTES, cap=5000, flags=flags)
            assert (A["result"], 32, "w") in r and (A["a2"], N_STR * rec, "w") in r and (A["a3"], 5000 * fields * rec, "w") in r
            assert ((A["feat"], 5000 * 25, "w") in r) == (what == FEATS)
            assert (A["utf8"], BYTES, "r") in r and (A["byte_off"], (N_STR + 1) * 8, "r") in r
            assert len(r) == (6 if what == FEATS else 5)
    # an empty batch still clears its result words, counts and row offsets on a slot's stream
    r = _ranges(OFFSETS, **A, n_str=N_STR, total_bytes=0, cap=5000)
    assert (A["result"], 32, "w") in r and (A["a2"], N_STR * 8, "w") in r
    assert (A["a3"], (N_STR + 1) * 8, "w") in _ranges(MASK, **A, n_str=N_STR, total_bytes=0, cap=0)


@pytest.mark.parametrize("what", [MASK, OFFSETS, SPANS, FEATS])
@pytest.mark.parametrize("shared", ["result", "a3", "a2", "utf8_written", None])
def test_a_second_batch_that_shares_one_output_is_ordered_behind_the_first(what, shared):
    """turn order would put the second batch on slot 1; sharing only the result words (any of the four), only cp_row_off / the
    records, only the mask / counts, or writing into the first one's input sends it to slot 0, behind the first"""
    submit, reset = _router()
    first = _ranges(what, **A, n_str=N_STR, total_bytes=BYTES, cap=5000)
    b = dict(B)
    if shared == "result":
        b["result"] = A["result"] + 24        # overlaps the LAST of the four result words only
    elif shared == "a3":
        b["a3"] = A["a3"] + (N_STR * 8 if what == MASK else 0)     # mask form: the last row offset only
    elif shared == "a2":
        b["a2"] = A["a2"]
    elif shared == "utf8_written":
        b["a3"] = A["utf8"] + 64              # its records / row offsets land in the bytes the first batch still reads
    second = _ranges(what, **b, n_str=N_STR, total_bytes=BYTES, cap=5000)
    assert submit(first) == (0, 0)
    assert submit(second) == ((1, 0) if shared is None else (0, 0))
    # ... also with an unrelated batch on the other slot in between; two batches that only READ the same input overlap freely
    reset()
    assert submit(first) == (0, 0)
    assert submit(_ranges(what, **{k: v + 0x40000000 for k, v in A.items()}, n_str=N_STR, total_bytes=BYTES, cap=5000)) == (1, 0)
    assert submit(second) == (0, 0)
    reset()
    same_input = dict(B, utf8=A["utf8"], byte_off=A["byte_off"])
    assert submit(first) == (0, 0)
    assert submit(_ranges(what, **same_input, n_str=N_STR, total_bytes=BYTES, cap=5000)) == (1, 0)
    reset()
