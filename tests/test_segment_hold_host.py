"""The constants of the tile kernel's held segments, from the built library (no device needed): latok_debug_tile_limits is a hook of
its own, latok_debug_limits stays closed at its 19 entries."""
import ctypes as C

import numpy as np


def _call(name, n):
    from latok_amd import _lib
    fn = getattr(_lib.load(), name)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.full(n, -1, np.int64)
    return fn(out.ctypes.data, n), out


def test_tile_limits():
    n, lim = _call("latok_debug_limits", 32)
    assert n == 19
    wpb, seg_max = int(lim[1]), int(lim[3])
    n, out = _call("latok_debug_tile_limits", 8)
    assert n == 2 and (out[2:] == -1).all()
    cap, lds_rounds = int(out[0]), int(out[1])
    # 12 rounds of the workgroup's waves; what is not held in LDS fits the 8 words a wave keeps in registers
    assert cap == 12 * wpb and cap <= seg_max
    assert 0 < lds_rounds and cap // wpb - lds_rounds <= 8
    assert _call("latok_debug_tile_limits", 1)[0] == 1
