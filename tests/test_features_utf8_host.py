"""UTF-8 featurize (latok_token_features_utf8_batch) without a GPU: argument checks of the Python wrappers and of the C entry
point, and no CPU fallback."""
import ctypes as C

import numpy as np
import pytest

from conftest import has_gpu


def test_python_argument_checks_need_no_device():
    from latok_amd import batch
    u8 = np.frombuffer("héllo wörld".encode(), np.uint8)
    for boff in (np.zeros(0, np.int64), np.array([0, u8.size + 1], np.int64), np.zeros((2, 2), np.int64)):
        with pytest.raises(ValueError):
            batch.token_features_utf8_csr(u8, boff)
    assert batch.featurize_utf8_batch([]) == []


def test_features_buffer_is_required_when_cap_is_positive():
    from latok_amd import _lib
    lib = _lib.load()
    u8 = np.frombuffer(b"ab cd", np.uint8)
    boff = np.array([0, 5], np.int64)
    counts, spans, n = np.zeros(1, np.int64), np.zeros((4, 4), np.int64), C.c_int64(0)
    rc = lib.latok_token_features_utf8_batch(u8.ctypes.data, boff.ctypes.data, 1, 5, counts.ctypes.data, spans.ctypes.data, None, 4,
                                             C.byref(n), 0, None)
    assert rc == _lib.ERR_INVALID and b"features_out" in lib.latok_last_error()


def test_no_cpu_fallback_without_device():
    if has_gpu():
        pytest.skip("a GPU is present")
    from latok_amd import _lib, batch
    lib = _lib.load()
    u8 = np.frombuffer("é日 x".encode(), np.uint8)
    boff = np.array([0, u8.size], np.int64)
    counts, spans, feats, n = np.zeros(1, np.int64), np.zeros((8, 4), np.int64), np.zeros((8, 25), np.int8), C.c_int64(0)
    rc = lib.latok_token_features_utf8_batch(u8.ctypes.data, boff.ctypes.data, 1, u8.size, counts.ctypes.data, spans.ctypes.data,
                                             feats.ctypes.data, 8, C.byref(n), 0, None)
    assert rc == _lib.ERR_NOT_INIT
    with pytest.raises(RuntimeError):
        batch.token_features_utf8_csr(u8, boff)
    with pytest.raises(RuntimeError):
        batch.featurize_utf8_batch([b"no gpu here"])
