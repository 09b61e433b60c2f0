"""Term keys (latok_amd/csrc/term_key.h; include/latok_hip.h: latok_term_counts_utf8_bytes_batch,
latok_hashed_term_counts_utf8_bytes_batch), the parts that need no device: term_key.h, compiled by g++ as a stand-alone program
(once more with the address and undefined-behaviour sanitizers) and run directly, gives the bucket and the sign of a Python
restatement of the rule -- key = |h| mod n_features in 64 bits, value = -1 iff alternate_sign and h < 0 -- for the edge hashes and
random ones; the vocabulary key orders ids as signed int32 and keeps "not found" behind and apart from every id; the restatement
is pinned to scikit-learn's FeatureHasher where that imports; the entry points exist in the library, the header and _lib.py with
one arity, and refuse bad arguments before they ask for a device."""
import ctypes as C
import os
import random
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

from helpers import murmur3_target as mt
from helpers.murmur3_ref import murmur3_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FEATURES = (1, 2, 3, 7, 64, 1 << 20, (1 << 31) - 1)
EDGE_HASHES = (0, 1, -1, (1 << 31) - 1, -(1 << 31), -(1 << 31) + 1)
ENTRIES = {"latok_term_counts_utf8_bytes_batch": 14, "latok_hashed_term_counts_utf8_bytes_batch": 15}


def restated(h, n_features, alternate_sign):
    """(column, value) of a token whose hash is h as int32: the rule of include/latok_hip.h, in Python's unbounded integers"""
    assert -(1 << 31) <= h < (1 << 31) and 1 <= n_features < (1 << 31)
    return abs(h) % n_features, (-1 if alternate_sign and h < 0 else 1)


def _i32(u):
    return u - (1 << 32) if u >= (1 << 31) else u


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    """the stand-alone program, built by plain g++ and once more with -fsanitize=address,undefined; it is run directly"""
    exe = tmp_path_factory.mktemp("term_key_" + request.param) / "term_key_harness"
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "term_key_harness.cpp"), "-o", str(exe)])

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
        rows = [r.split() for r in out.stdout.splitlines()]
        assert len(rows) == len(lines)
        return [(int(k, 16), int(c), int(v), int(o), int(h, 16)) for k, c, v, o, h in rows]

    return run


def test_bucket_and_sign_follow_the_restated_rule(harness):
    rng = random.Random(12)
    hashes = list(EDGE_HASHES) + [_i32(rng.getrandbits(32)) for _ in range(500)]
    cases = [(h, n, alt) for n in N_FEATURES for alt in (0, 1) for h in hashes]
    got = harness(["h %x %d %d" % (h & 0xFFFFFFFF, n, alt) for h, n, alt in cases])
    for (h, n, alt), (key, col, val, oov, _) in zip(cases, got):
        assert (col, val) == restated(h, n, bool(alt)), (h, n, alt, col, val)
        assert oov == 0 and key >> 34 == 0 and 0 <= col < n
    # the one hash whose magnitude does not fit int32
    assert restated(-(1 << 31), 7, True) == ((1 << 31) % 7, -1) and restated(-(1 << 31), (1 << 31) - 1, False) == (1, 1)


def test_hashed_keys_of_one_column_differ_in_the_sign_bit_only_and_sort_by_column(harness):
    rng = random.Random(13)
    hashes = list(EDGE_HASHES) + [_i32(rng.getrandbits(32)) for _ in range(300)]
    for n in (2, 7, 1 << 20, (1 << 31) - 1):
        got = harness(["h %x %d 1" % (h & 0xFFFFFFFF, n) for h in hashes])
        by_key = sorted(got)
        assert [c for _, c, _, _, _ in by_key] == sorted(c for _, c, _, _, _ in got)           # ascending keys = ascending columns
        entry = {}
        for key, col, val, _, _ in got:
            assert entry.setdefault(key >> 1, col) == col and (key & 1) == (val < 0)


def test_vocabulary_keys_order_ids_as_signed_int32_and_keep_not_found_apart(harness):
    rng = random.Random(14)
    ids = [-(1 << 31), -1, 0, 1, 255, 256, 65535, 65536, 1 << 24, (1 << 31) - 1] + [_i32(rng.getrandbits(32)) for _ in range(300)]
    got = harness(["v %d" % i for i in ids] + ["o"])
    keys = [k for k, _, _, _, _ in got[:-1]]
    assert [c for _, c, _, _, _ in got[:-1]] == ids and all(v == 1 and o == 0 for _, _, v, o, _ in got[:-1])
    assert [i for _, i in sorted(zip(keys, ids))] == sorted(ids)
    oov_key, _, _, oov, _ = got[-1]
    assert oov == 1 and oov_key > max(keys) and oov_key >> 34 == 0
    assert len({k >> 1 for k in keys}) == len(set(ids))                                        # an id equal to -1 is an id like any other


def test_the_crafted_token_hashes_to_int32_min_in_both_implementations(harness):
    tok = mt.INT32_MIN_TOKEN
    assert mt.token_with_hash(0x80000000, 0) == tok and murmur3_ref(tok, 0) == 0x80000000
    assert not any(b in b" \t\n\r\x0b\x0c" for b in tok) and len(tok) == 8
    for n in N_FEATURES:
        for alt in (0, 1):
            (key, col, val, oov, h), = harness(["t 0 %d %d %s" % (n, alt, tok.hex())])
            assert h == murmur3_ref(tok, 0) == 0x80000000
            assert (col, val) == restated(-(1 << 31), n, bool(alt)) == ((1 << 31) % n, -1 if alt else 1)
    words = [b"a", b"ab", b"abc", b"abcd", b"hello", b"tokenizer", bytes(range(33, 60))]
    got = harness(["t %x 64 1 %s" % (seed, w.hex()) for seed in (0, 1, 0x9747B28C) for w in words])
    assert [g[4] for g in got] == [murmur3_ref(w, seed) for seed in (0, 1, 0x9747B28C) for w in words]
    assert mt.unfmix32(0) == 0 and all(murmur3_ref(mt.token_with_hash(t, s), s) == t for t, s in ((0, 0), (0xFFFFFFFF, 5), (0x12345678, 1)))


def _rows(rng, n_rows):
    """rows of short tokens over a small alphabet: collisions inside a row at every n_features"""
    return [["".join(rng.choice("abcdefgh") for _ in range(rng.randint(1, 3))) for _ in range(rng.randint(0, 40))] for _ in range(n_rows)]


def test_the_restatement_is_scikit_learns_feature_hasher():
    pytest.importorskip("sklearn")
    from sklearn.feature_extraction import FeatureHasher
    rows = _rows(random.Random(15), 300)
    for n in N_FEATURES:
        for alt in (False, True):
            m = FeatureHasher(n_features=n, input_type="string", dtype=np.int64, alternate_sign=alt).transform(rows)
            m.sum_duplicates()
            m.sort_indices()
            zeros = 0
            for s, row in enumerate(rows):
                want = Counter()
                for t in row:
                    col, val = restated(_i32(murmur3_ref(t.encode(), 0)), n, alt)
                    want[col] += val
                lo, hi = m.indptr[s], m.indptr[s + 1]
                assert m.indices[lo:hi].tolist() == sorted(want) and m.data[lo:hi].tolist() == [want[c] for c in sorted(want)], (n, alt, s)
                zeros += sum(v == 0 for v in want.values())
            if alt and n <= 64:
                assert zeros > 0, (n, "explicit zeros are kept")


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
    for name in ("term_counts_utf8_csr", "term_counts_utf8_batch", "term_counts_batch", "hashed_term_counts_utf8_csr",
                 "hashed_term_counts_utf8_batch", "hashed_term_counts_batch"):
        assert callable(getattr(batch, name)), name
    assert "scipy.sparse.csr_matrix((data, indices, indptr), shape=(n, n_cols))" in batch.term_counts_utf8_csr.__doc__


def test_limits_report_the_tile_and_the_longest_short_row():
    from latok_amd import _lib
    fn = _lib.load().latok_debug_terms_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(4, np.int64)
    assert fn(out.ctypes.data, 4) == 2 and fn(out.ctypes.data, 1) == 1
    tile, row_max = int(out[0]), int(out[1])
    assert tile >= 64 and tile & (tile - 1) == 0 and 1 <= row_max <= tile


def test_header_with_the_new_calls_is_c99_and_the_example_compiles(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "latok_hip.h"\n'
                   "int f(const uint8_t* u, const int64_t* o, latok_vocab* v, int64_t* ip, int64_t* oov, int32_t* ix, int32_t* d, int64_t* n) {\n"
                   "    int rc = latok_term_counts_utf8_bytes_batch(u, o, 1, -1, v, ip, oov, ix, d, 64, n, NULL, 0, NULL);\n"
                   "    rc += latok_term_counts_utf8_bytes_batch(u, o, 1, -1, v, ip, NULL, NULL, NULL, 0, n, n + 1, LATOK_OUT_INT32, NULL);\n"
                   "    return rc + latok_hashed_term_counts_utf8_bytes_batch(u, o, 1, -1, 0u, 1 << 20, 1, ip, ix, d, 64, n, NULL, 0, NULL);\n}\n")
    strict = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c"]
    subprocess.check_call(strict + [str(src), "-o", str(tmp_path / "use.o")])
    subprocess.check_call(strict + [os.path.join(ROOT, "examples", "term_counts_utf8.c"), "-o", str(tmp_path / "example.o")])


def test_python_wrappers_refuse_bad_arguments_before_any_device():
    from latok_amd import batch
    for bad in (0, -1, 1 << 31, 2.0, True, None):
        with pytest.raises(ValueError):
            batch.hashed_term_counts_utf8_batch([b"a b"], n_features=bad)
    for bad in (-1, 1 << 32, "0"):
        with pytest.raises(ValueError):
            batch.hashed_term_counts_batch(["a b"], seed=bad)
    with pytest.raises(ValueError):
        batch.term_counts_utf8_batch([b"a b"], vocab=None)
    with pytest.raises(ValueError):
        batch.hashed_term_counts_utf8_csr(np.zeros(3, np.uint8), np.array([0, 3]), dtype=np.int16)
