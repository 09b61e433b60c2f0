"""TF-IDF (include/latok_hip.h: latok_idf_*, latok_tfidf_csr, latok_tfidf_utf8_bytes_batch, latok_hashed_tfidf_utf8_bytes_batch), the
parts that need no device: tfidf_weight.h, compiled by g++ as a stand-alone program (once more with the address and
undefined-behaviour sanitizers), gives the idf, tf and scaling of tests/helpers/tfidf_ref.py within 8 * 2^-23 relative, with exact
zeros where the rule says zero; the reference itself equals scikit-learn's TfidfTransformer in float64 wherever that is defined; the
entry points exist in the library, the header and latok_amd/_lib.py with one arity; what is refused before any device work is refused
without a device."""
import ctypes as C
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from helpers import tfidf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"latok_idf_create": 2, "latok_idf_destroy": 1, "latok_idf_clear": 1, "latok_idf_info": 4, "latok_idf_update_csr": 7,
           "latok_idf_update_utf8_bytes_batch": 15, "latok_idf_read": 4, "latok_idf_load": 3, "latok_idf_weights": 4, "latok_tfidf_csr": 10,
           "latok_tfidf_utf8_bytes_batch": 18, "latok_hashed_tfidf_utf8_bytes_batch": 19}
BOUND = 8 * ref.EPS


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def lines(request, tmp_path_factory):
    """what the stand-alone program prints, built by plain g++ and once more with -fsanitize=address,undefined; it is run directly"""
    exe = tmp_path_factory.mktemp("tfidf_" + request.param) / "tfidf_harness"
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I" + os.path.join(ROOT, "latok_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "tfidf_harness.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return [line.split() for line in out.stdout.splitlines()]


def _f32(hexbits):
    return float(np.float32(struct.unpack("<f", struct.pack("<I", int(hexbits, 16)))[0]))


def _close(got, want, bound=BOUND):
    if want == 0:
        return got == 0
    return np.isfinite(got) and abs(got - want) <= bound * abs(want)


def test_idf_rule(lines):
    seen = set()
    for kind, *f in lines:
        if kind != "idf":
            continue
        df, n, smooth, got = int(f[0]), int(f[1]), int(f[2]), _f32(f[3])
        want = float(ref.idf(np.array([df]), n, bool(smooth))[0])
        assert _close(got, want), (df, n, smooth, got, want)
        seen.add((df, n, smooth))
    n_max = 2 ** 31 - 1
    assert seen == {(df, n, s) for s in (0, 1) for n in (0, 1, n_max) for df in (0, 1, n) if df <= n}
    # the unsmoothed zero column is 0 (scikit-learn divides by zero there); one document that holds the column: ln 1 + 1
    assert ref.idf(np.array([0]), 5, False)[0] == 0 and ref.idf(np.array([1]), 1, False)[0] == 1.0


def test_tf_rule(lines):
    seen = set()
    for kind, *f in lines:
        if kind != "tf":
            continue
        t, sub, got = int(f[0]), int(f[1]), _f32(f[2])
        want = float(ref.tf(np.array([t]), bool(sub))[0])
        assert _close(got, want), (t, sub, got, want)
        if t == 0:
            assert f[2] == "00000000"
        seen.add((t, sub))
    ts = (-(2 ** 31) + 1, -3, -1, 0, 1, 2, 2 ** 24 + 1, 2 ** 31 - 1)
    assert seen == {(t, s) for t in ts for s in (0, 1)}


def test_scaling_rule(lines):
    """tw_term / tw_norm / tw_scale over one row: the reference's row within (k + 16) * 2^-23, a zero row keeps its zeros, and a single
    entry under L2 is exactly 1"""
    n = 0
    for kind, *f in lines:
        if kind != "row":
            continue
        norm, k, zeros = (None, "l1", "l2")[int(f[0])], int(f[1]), int(f[2])
        got = np.array([_f32(x) for x in f[3:]])
        data = np.zeros(k) if zeros else np.array([(i + 1) * (-1 if i & 1 else 1) for i in range(k)], np.float64)
        want = ref.weigh([0, k], np.arange(k), data, None, False, norm)
        assert ref.worst(got, want, [0, k], norm)[0] <= 1, (norm, k, zeros, got, want)
        if zeros:
            assert all(x == "00000000" for x in f[3:])
        if norm == "l2" and k == 1 and not zeros:
            assert f[3] == "3f800000"
        n += 1
    assert n == 18


@pytest.mark.parametrize("smooth_idf,sublinear_tf,norm", list(itertools.product((False, True), (False, True), ("l1", "l2", None))))
def test_reference_is_tfidf_transformer(smooth_idf, sublinear_tf, norm):
    """tfidf_ref.py against scikit-learn in float64, 1e-12 relative, on a random non-negative CSR whose every column occurs: the domain
    where scikit-learn is defined"""
    pytest.importorskip("sklearn")
    sp = pytest.importorskip("scipy.sparse")
    from sklearn.feature_extraction.text import TfidfTransformer
    rng = np.random.default_rng(7)
    n_rows, n_cols = 23, 11
    dense = rng.integers(1, 9, (n_rows, n_cols)) * (rng.random((n_rows, n_cols)) < 0.4)
    dense[rng.integers(0, n_rows, n_cols), np.arange(n_cols)] = 3   # every column occurs at least once
    dense[5] = 0                                                      # an empty row
    X = sp.csr_matrix(dense.astype(np.float64))
    X.sort_indices()
    want = TfidfTransformer(norm=norm, use_idf=True, smooth_idf=smooth_idf, sublinear_tf=sublinear_tf).fit_transform(X.copy())
    want.sort_indices()
    idf = ref.idf(ref.document_frequency(X.indices, n_cols), n_rows, smooth_idf)
    got = ref.weigh(X.indptr, X.indices, X.data, idf, sublinear_tf, norm)
    assert np.array_equal(want.indptr, X.indptr) and np.array_equal(want.indices, X.indices)
    assert np.allclose(got, want.data, rtol=1e-12, atol=0)


def _header():
    text = open(os.path.join(ROOT, "include", "latok_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_entry_points_have_one_arity():
    from latok_amd import _lib
    lib = _lib.load()
    text = _header()
    for name, arity in ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, "%s is not declared in include/latok_hip.h" % name
        assert len(m.group(1).split(",")) == arity, name
        assert len(_lib.SIGNATURES[name][1]) == arity, name
        assert getattr(lib, name) is not None
    for name, value in (("SMOOTH_IDF", 1), ("SUBLINEAR_TF", 2), ("NORM_L1", 4), ("NORM_L2", 8)):
        assert re.search(r"#define\s+LATOK_TFIDF_%s\s+%d\b" % (name, value), text) and getattr(_lib, "TFIDF_" + name) == value
    limits = (C.c_int64 * 3)()
    assert lib.latok_debug_tfidf_limits(limits, 3) == 3 and 0 < limits[0] < limits[1] and limits[2] > 0


def test_refusals_before_any_device_work():
    """n_cols out of range, both norm bits, an unknown opts bit, an unknown flag: refused whether or not a device exists, nothing
    written"""
    from latok_amd import _lib
    lib = _lib.load()
    h = C.c_void_p(0x1234)
    for n_cols in (0, -1, 2 ** 28 + 1):
        assert lib.latok_idf_create(n_cols, C.byref(h)) == _lib.ERR_INVALID and b"n_cols" in lib.latok_last_error()
        assert not h.value
        h = C.c_void_p(0x1234)
    indptr, indices, data = np.array([0, 1], np.int64), np.array([0], np.int32), np.array([2], np.int32)
    out = np.full(1, 7.0, np.float32)
    for opts in (4 | 8, 16, -1):
        rc = lib.latok_tfidf_csr(indptr.ctypes.data, indices.ctypes.data, data.ctypes.data, 1, 1, None, opts, out.ctypes.data, 0, None)
        assert rc == _lib.ERR_INVALID and out[0] == 7.0
    assert lib.latok_tfidf_csr(indptr.ctypes.data, indices.ctypes.data, data.ctypes.data, 1, 1, None, 0, out.ctypes.data, 4, None) == _lib.ERR_INVALID
    assert b"unknown flag" in lib.latok_last_error() and out[0] == 7.0
    u8, off, nnz = np.frombuffer(b"a b", np.uint8), np.array([0, 3], np.int64), C.c_int64(5)
    ip = np.full(2, 9, np.int64)
    rc = lib.latok_hashed_tfidf_utf8_bytes_batch(u8.ctypes.data, off.ctypes.data, 1, 3, 0, 16, 1, 1, 1, 32, None, 12, ip.ctypes.data, None, None, 0,
                                                 C.byref(nnz), 0, None)
    assert rc == _lib.ERR_INVALID and ip.tolist() == [9, 9]
    from latok_amd import batch
    with pytest.raises(ValueError):
        batch.tfidf_csr(indptr, indices, data, norm="max")
