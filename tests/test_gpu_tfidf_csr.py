"""latok_tfidf_csr and latok_idf_update_csr (include/latok_hip.h) on CSRs that a caller built (tests/helpers/csr_cases.py), where
test_gpu_tfidf.py only hands them what the library's own count kernels wrote: long rows at every position relative to the tiles of
k_tfidf_long, every mixture of tiers inside one wave of k_tfidf_rows, zeros, mixed signs, INT32_MIN / INT32_MAX and counts above 2^24
in the wave and workgroup tiers, spike rows (one entry of 1000 among ones: a skipped or repeated entry cannot hide under the bound),
device pointers at every 4-byte offset, CSRs beyond the 2048 x 256 threads of the grid-stride kernels, two hot columns in one LDS slot
of k_df_add, repeated columns.

No tolerance of its own: outputs are held to tests/helpers/tfidf_ref.py (numpy float64) under the header's bounds -- (k + 16) * 2^-23
relative for a normalised row of k entries, 8 * 2^-23 without a norm, exact zeros where the rule says zero -- and idf vectors to 2^-24
of the largest weight, as in test_gpu_tfidf.py.  test_csr_cases_host.py shows, without a device, that the expected values are what
these tests take them for.  Every test prints the worst error over its bound that it met."""
import ctypes as C

import numpy as np
import pytest

from helpers import csr_cases as cc
from helpers import tfidf_ref as ref

pytestmark = pytest.mark.gpu

POISON = 0xA5
U32 = np.uint32
ONE, MINUS_ONE = 0x3F800000, 0xBF800000


@pytest.fixture(scope="module")
def idf(gpu):
    """an Idf of N_COLS columns loaded with a fixed random df that has zero columns; no test may change it"""
    from latok_amd import batch
    df, n_docs = cc.fixed_df()
    with batch.Idf(cc.N_COLS) as f:
        f.load(df, n_docs)
        yield f
        assert np.array_equal(f.df(), df) and f.n_docs == n_docs


@pytest.fixture(scope="module")
def idf_vec():
    df, n_docs = cc.fixed_df()
    return {smooth: ref.idf(df, n_docs, smooth) for smooth in (False, True)}


def _opts(smooth, sub, norm):
    from latok_amd import batch
    return batch._tfidf_opts(smooth, sub, norm)


def _want(csr, vec, sub, norm):
    """the float64 reference: tfidf_ref.weigh, or for a CSR of many rows its vectorised twin"""
    return (cc.weigh if csr[0].size > 5000 else ref.weigh)(csr[0], csr[1], csr[2], vec, sub, norm)


def _hold(got, csr, vec, sub, norm, what, want=None):
    """-> worst error over its bound"""
    assert got.dtype == np.float32 and got.shape == csr[2].shape, what
    want = _want(csr, vec, sub, norm) if want is None else want
    w, i = ref.worst(got, want, csr[0], norm)
    assert w <= 1, (what, "entry %d: got %r, want %r, %.2f of the bound" % (i, got[i], want[i], w))
    assert np.isfinite(got).all() and (got.view(U32)[csr[2] == 0] == 0).all(), what     # a zero count: +0.0f
    return w


def _sweep(csr, idf, idf_vec, opts, what, widths=(np.int64, np.int32)):
    """every option combination with the idf, the norms and tf rules once more without; both widths of indptr -> worst ratio"""
    from latok_amd import batch
    worst = 0.0
    runs = [(idf, s, t, n) for s, t, n in opts] + [(None, True, t, n) for t, n in sorted({o[1:] for o in opts}, key=str)]
    for f, smooth, sub, norm in runs:
        bits, want = None, _want(csr, idf_vec[smooth] if f else None, sub, norm)
        for dt in widths:
            got = batch.tfidf_csr(csr[0].astype(dt), csr[1], csr[2], f, smooth, sub, norm)
            worst = max(worst, _hold(got, csr, None, sub, norm, (what, f is not None, smooth, sub, norm, dt.__name__), want))
            assert bits is None or np.array_equal(bits, got.view(U32)), (what, "the two widths of indptr differ")
            bits = got.view(U32)
    return worst


def _report(case, worst):
    print("\n[tfidf_csr] %s: worst error %.3f of the bound" % (case, worst))


# ---- device buffers --------------------------------------------------------------------------------------------------
class Dev:
    """device buffers of one test from latok_dev_alloc, poisoned around what they hold, freed together"""

    def __init__(self, lib):
        self.lib, self.bufs = lib, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for base, _ in self.bufs:
            self.lib.latok_dev_free(base)
        return False

    def put(self, a, offset=0, slack=64):
        """a copy of the array `offset` bytes behind a 16-byte boundary, POISON in front and behind -> its device address"""
        from latok_amd import _lib
        a = np.ascontiguousarray(a)
        size = 16 + a.nbytes + slack
        base = self.lib.latok_dev_alloc(size)
        assert base and base % 16 == 0 and 0 <= offset < 16
        self.bufs.append((base, size))
        host = np.full(size, POISON, np.uint8)
        host[offset:offset + a.nbytes] = a.view(np.uint8).ravel()
        _lib.check(self.lib.latok_memcpy_h2d(base, host.ctypes.data, size))
        return base + offset

    def get(self, p, n, dtype):
        from latok_amd import _lib
        out = np.empty(n, dtype)
        if n:
            _lib.check(self.lib.latok_memcpy_d2h(out.ctypes.data, p, out.nbytes))
        return out

    def poison_intact(self, p, nbytes):
        """the bytes in front of p back to its allocation's start and behind p + nbytes up to its end"""
        base, size = next(b for b in self.bufs if b[0] <= p < b[0] + b[1])
        raw = self.get(base, size, np.uint8)
        return (raw[:p - base] == POISON).all() and (raw[p - base + nbytes:] == POISON).all()

    def set(self, p, value, dtype):
        from latok_amd import _lib
        v = np.array([value], dtype)
        _lib.check(self.lib.latok_memcpy_h2d(p, v.ctypes.data, v.nbytes))


def _dev_tfidf(lib, indptr_p, indices_p, data_p, n_rows, nnz, idf, opts, out_p, ip32=False):
    from latok_amd import _lib
    return lib.latok_tfidf_csr(indptr_p, indices_p, data_p, n_rows, nnz, idf.handle if idf else None, opts, out_p,
                               _lib.DEVICE_PTRS | (_lib.OUT_INT32 if ip32 else 0), None)


# ---- 1: where a long row sits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.LONG_ROW_NAMES)
def test_long_row_placement(idf, idf_vec, name):
    S, W, SLOTS = cc.limits()
    csr = cc.long_row_case(name, S, W)
    lens = np.diff(csr[0])
    assert lens.tolist() == cc.long_row_layouts(S, W)[name] and lens.max() > W
    _report("long-row placement " + name, _sweep(csr, idf, idf_vec, cc.OPTS if csr[2].size < 20000 else cc.OPTS_FEW, name))


# ---- 2: the tiers inside one wave ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.WAVE_NAMES)
def test_tiers_inside_one_wave(idf, idf_vec, name):
    S, W, SLOTS = cc.limits()
    csr = cc.wave_case(name, S, W)
    assert np.diff(csr[0]).tolist() == cc.wave_layouts(S, W)[name]
    _report("tiers inside one wave " + name, _sweep(csr, idf, idf_vec, cc.OPTS, name))


# ---- 3: every kind of data in every tier -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cc.KINDS)
def test_data_kinds_in_every_tier(idf, idf_vec, kind):
    from latok_amd import batch
    S, W, SLOTS = cc.limits()
    csr = cc.kind_case(kind, S, W)
    assert np.diff(csr[0]).tolist() == cc.tier_lengths(S, W)
    _report("data kind " + kind, _sweep(csr, idf, idf_vec, cc.OPTS, kind))
    if kind == "zeros":
        for smooth, sub, norm in cc.OPTS:
            for f in (idf, None):
                assert not batch.tfidf_csr(*csr, f, smooth, sub, norm).view(U32).any()      # every entry the bits of +0.0f
    if kind == "extreme":
        assert {cc.I32_MIN, cc.I32_MAX, cc.BIG, 0} <= set(csr[2][csr[0][-2]:].tolist())         # the long row holds them all


# ---- 4: spike rows ---------------------------------------------------------------------------------------------------
def test_spike_rows(gpu):
    """no idf; test_csr_cases_host.py shows that one skipped or repeated spike moves its row by more than 100 bounds"""
    from latok_amd import batch
    S, W, SLOTS = cc.limits()
    csr = cc.spike_case(S, W)
    worst = 0.0
    for sub in (False, True):
        for norm in ("l2", "l1", None):
            for dt in (np.int64, np.int32):
                got = batch.tfidf_csr(csr[0].astype(dt), csr[1], csr[2], None, True, sub, norm)
                worst = max(worst, _hold(got, csr, None, sub, norm, ("spike", sub, norm)))
    _report("spike rows", worst)


# ---- 5: single-entry rows under L2 -----------------------------------------------------------------------------------
def test_single_entry_rows_are_plus_or_minus_one(idf, idf_vec):
    from latok_amd import batch
    csr = cc.single_entry_case()
    assert set(csr[2].tolist()) == set(cc.SINGLE_COUNTS) and csr[1].min() == 0 and csr[1].max() == cc.N_COLS - 1
    worst = 0.0
    for f in (idf, None):
        for smooth in (False, True):
            for sub in (False, True):
                vec = idf_vec[smooth] if f else None
                got = batch.tfidf_csr(*csr, f, smooth, sub, "l2")
                worst = max(worst, _hold(got, csr, vec, sub, "l2", ("single", f is not None, smooth, sub)))
                zero = (vec[csr[1]] == 0) if f else np.zeros(csr[2].size, bool)
                assert (f is None or smooth) != bool(zero.any())                             # the zero weights of the unsmoothed idf
                want = np.where(zero, 0, np.where(csr[2] < 0, MINUS_ONE, ONE)).astype(U32)
                bad = np.nonzero(got.view(U32) != want)[0]
                assert bad.size == 0, ("count %d, column %d gives %r" % (csr[2][bad[0]], csr[1][bad[0]], got[bad[0]]), f is not None, smooth, sub)
    _report("single-entry rows", worst)


# ---- 6: a row's bits depend on the row alone -------------------------------------------------------------------------
def test_row_bits_do_not_depend_on_the_placement(idf, idf_vec, gpu):
    from latok_amd import batch
    S, W, SLOTS = cc.limits()
    rows = cc.independence_rows(S, W)
    worst = 0.0
    for smooth, sub, norm in ((True, True, "l2"), (False, False, "l1"), (True, False, None)):
        alone = []
        for r in rows:                                                                       # every row as a batch of its own
            one = cc.build([r])
            got = batch.tfidf_csr(*one, idf, smooth, sub, norm)
            worst = max(worst, _hold(got, one, idf_vec[smooth], sub, norm, ("alone", r[0].size)))
            alone.append(got.view(U32))
        together = batch.tfidf_csr(*cc.build(rows), idf, smooth, sub, norm).view(U32)       # back to back, no filler
        assert np.array_equal(together, np.concatenate(alone))
        for b in (1, 2, 3):
            csr, where = cc.independence_batch(rows, b, S, W)
            got = batch.tfidf_csr(*csr, idf, smooth, sub, norm)
            worst = max(worst, _hold(got, csr, idf_vec[smooth], sub, norm, ("batch", b)))
            results = [got.view(U32), batch.tfidf_csr(csr[0].astype(np.int32), csr[1], csr[2], idf, smooth, sub, norm).view(U32)]
            if b == 1:                                                                       # once more through device pointers
                with Dev(gpu) as dev:
                    p = [dev.put(a) for a in csr]
                    out = dev.put(np.zeros(csr[2].size, np.float32))
                    assert _dev_tfidf(gpu, p[0], p[1], p[2], csr[0].size - 1, csr[2].size, idf, _opts(smooth, sub, norm), out) == 0
                    results.append(dev.get(out, csr[2].size, U32))
            for res in results:
                for i, w in enumerate(where):
                    a = int(csr[0][w])
                    assert np.array_equal(res[a:a + alone[i].size], alone[i]), (b, rows[i][0].size, smooth, sub, norm)
    _report("row independence", worst)


# ---- 7: pointers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [(0, 0, 0), (4, 8, 12), (8, 12, 4), (12, 4, 8), (12, 12, 12)])
def test_device_pointers_at_every_offset(idf, gpu, offsets):
    """indices, data and data_out at 0, 4, 8 and 12 bytes behind a 16-byte boundary; out of place and in place"""
    from latok_amd import _lib, batch
    S, W, SLOTS = cc.limits()
    csr = cc.pointer_case(S, W)
    n_rows, nnz = csr[0].size - 1, csr[2].size
    for smooth, sub, norm in cc.OPTS_FEW:
        opts = _opts(smooth, sub, norm)
        host = batch.tfidf_csr(*csr, idf, smooth, sub, norm).view(U32)
        for ip32 in (False, True):
            with Dev(gpu) as dev:
                ip = dev.put(csr[0].astype(np.int32) if ip32 else csr[0])
                ix, d, out = dev.put(csr[1], offsets[0]), dev.put(csr[2], offsets[1]), dev.put(np.full(nnz, 7.0, np.float32), offsets[2])
                assert _dev_tfidf(gpu, ip, ix, d, n_rows, nnz, idf, opts, out, ip32) == 0, _lib.last_error()    # out of place
                assert np.array_equal(dev.get(out, nnz, U32), host)
                assert np.array_equal(dev.get(d, nnz, np.int32), csr[2]) and np.array_equal(dev.get(ix, nnz, np.int32), csr[1])
                assert dev.poison_intact(out, 4 * nnz) and dev.poison_intact(d, 4 * nnz) and dev.poison_intact(ix, 4 * nnz)
                assert _dev_tfidf(gpu, ip, ix, d, n_rows, nnz, idf, opts, d, ip32) == 0, _lib.last_error()      # in place
                assert np.array_equal(dev.get(d, nnz, U32), host) and dev.poison_intact(d, 4 * nnz)


def test_host_pointers_in_place_and_a_misaligned_device_output(idf, gpu):
    from latok_amd import _lib, batch
    S, W, SLOTS = cc.limits()
    csr = cc.pointer_case(S, W)
    n_rows, nnz = csr[0].size - 1, csr[2].size
    for smooth, sub, norm in cc.OPTS_FEW:
        want = batch.tfidf_csr(*csr, idf, smooth, sub, norm).view(U32)
        both = csr[2].copy()                                                                 # one buffer, int32 in and float32 out
        rc = gpu.latok_tfidf_csr(csr[0].ctypes.data, csr[1].ctypes.data, both.ctypes.data, n_rows, nnz, idf.handle, _opts(smooth, sub, norm),
                                 both.ctypes.data, 0, None)
        assert rc == 0 and np.array_equal(both.view(U32), want)
    with Dev(gpu) as dev:
        p = [dev.put(a) for a in csr]
        out = dev.put(np.full(nnz, 7.0, np.float32))
        for off in (1, 2, 3):
            assert _dev_tfidf(gpu, p[0], p[1], p[2], n_rows, nnz, idf, 9, out + off) == _lib.ERR_INVALID and "misaligned" in _lib.last_error()
        assert (dev.get(out, nnz, np.float32) == 7.0).all() and dev.poison_intact(out, 4 * nnz)


# ---- 8: latok_idf_update_csr through device pointers ------------------------------------------------------------------
@pytest.mark.parametrize("cached", [1, 0], ids=["lds_table", "plain"])
def test_df_of_two_hot_columns_in_one_slot(gpu, cached):
    """3 * 16384 + 5 entries, so three whole chunks of k_df_add and a tail; indices at 0, 4, 8 and 12 bytes behind a 16-byte boundary: at
    the last three every chunk starts with the scalar head of df_for_each, of 3, 2 and 1 entries"""
    from latok_amd import _lib, batch
    S, W, SLOTS = cc.limits()
    indptr, indices, n_cols, (a, b), own = cc.df_collision_case(SLOTS)
    n_rows = indptr.size - 1
    want = np.bincount(indices, minlength=n_cols)
    assert want[a] == want[b] == n_rows - 1 and want[0] == want[n_cols - 1] == 1
    gpu.latok_debug_set_df_add.restype, gpu.latok_debug_set_df_add.argtypes = C.c_int, [C.c_int]
    gpu.latok_debug_set_df_add(cached)
    try:
        with batch.Idf(n_cols) as host:
            host.update_csr(indptr, indices)
            assert np.array_equal(host.df(), want) and host.n_docs == n_rows
            host.update_csr(indptr.astype(np.int32), indices)
            assert np.array_equal(host.df(), 2 * want) and host.n_docs == 2 * n_rows
        for offset in (0, 4, 8, 12):
            with batch.Idf(n_cols) as f, Dev(gpu) as dev:
                ip, ix = dev.put(indptr), dev.put(indices, offset)
                _lib.check(gpu.latok_idf_update_csr(f.handle, ip, ix, n_rows, indices.size, _lib.DEVICE_PTRS, None))
                assert np.array_equal(f.df(), want) and f.n_docs == n_rows, offset
                assert np.array_equal(dev.get(ix, indices.size, np.int32), indices) and dev.poison_intact(ix, indices.nbytes)
                tail = indices.size - 7                                                      # a second batch: an odd start, an odd length
                ip1 = dev.put(np.array([0, tail], np.int64))
                _lib.check(gpu.latok_idf_update_csr(f.handle, ip1, ix + 12, 1, tail, _lib.DEVICE_PTRS, None))
                assert np.array_equal(f.df(), want + np.bincount(indices[3:3 + tail], minlength=n_cols)) and f.n_docs == n_rows + 1
    finally:
        gpu.latok_debug_set_df_add(1)


# ---- 9: beyond the stride limit of k_csr_check and k_idf_weights ------------------------------------------------------
def test_600001_rows_and_defects_behind_the_stride_limit(idf, idf_vec, gpu):
    from latok_amd import _lib, batch
    csr = cc.stride_case()
    indptr, indices, data = csr
    n_rows, nnz = indptr.size - 1, data.size
    assert n_rows == nnz == 600001 > cc.STRIDE_LIMIT
    worst = 0.0
    for smooth, sub, norm in ((True, False, "l2"), (False, True, "l2"), (True, True, None), (False, False, None)):
        got = batch.tfidf_csr(*csr, idf, smooth, sub, norm)
        worst = max(worst, _hold(got, csr, idf_vec[smooth], sub, norm, ("stride", smooth, sub, norm)))
    _report("600 001 rows", worst)
    with Dev(gpu) as dev, batch.Idf(cc.N_COLS) as counted:
        counted.update_csr(indptr, indices)
        assert np.array_equal(counted.df(), np.bincount(indices, minlength=cc.N_COLS)) and counted.n_docs == n_rows
        p_ip, p_ix, p_d = (dev.put(a) for a in csr)
        p_out = dev.put(np.full(nnz, 7.0, np.float32))
        for name, (ip, ix, words) in cc.stride_defects(indptr, indices, cc.N_COLS).items():
            for use in (idf, None) if words != "column" else (idf,):                     # without an idf any int32 is a column
                with pytest.raises(ValueError, match=words):
                    batch.tfidf_csr(ip, ix, data, use)
                out = np.full(nnz, 7.0, np.float32)
                rc = gpu.latok_tfidf_csr(ip.ctypes.data, ix.ctypes.data, data.ctypes.data, n_rows, nnz, use.handle if use else None, 9,
                                         out.ctypes.data, 0, None)
                assert rc == _lib.ERR_INVALID and words in _lib.last_error() and (out == 7.0).all(), name
            with pytest.raises(ValueError, match=words):
                counted.update_csr(ip, ix)
            with pytest.raises(ValueError, match=words):
                counted.update_csr(ip.astype(np.int32), ix)
            # the same defect in the device copy: one element changed, the call, the element put back
            p, src, orig = (p_ip, ip, indptr) if (ip != indptr).any() else (p_ix, ix, indices)
            (i,) = np.nonzero(src != orig)[0]
            dev.set(p + int(i) * src.itemsize, src[i], src.dtype)
            assert _dev_tfidf(gpu, p_ip, p_ix, p_d, n_rows, nnz, idf, 9, p_out) == _lib.ERR_INVALID and words in _lib.last_error(), name
            rc = gpu.latok_idf_update_csr(counted.handle, p_ip, p_ix, n_rows, nnz, _lib.DEVICE_PTRS, None)
            assert rc == _lib.ERR_INVALID and words in _lib.last_error(), name
            dev.set(p + int(i) * src.itemsize, orig[i], src.dtype)
            assert (dev.get(p_out, nnz, np.float32) == 7.0).all() and np.array_equal(dev.get(p_d, nnz, np.int32), data), name
        assert np.array_equal(counted.df(), np.bincount(indices, minlength=cc.N_COLS)) and counted.n_docs == n_rows
        assert _dev_tfidf(gpu, p_ip, p_ix, p_d, n_rows, nnz, idf, 9, p_out) == 0             # the device copy is whole again
        assert np.array_equal(dev.get(p_out, nnz, U32), batch.tfidf_csr(*csr, idf).view(U32))


def test_more_rows_than_entries(idf, idf_vec, gpu):
    """600 000 rows, 5 entries: the span of k_csr_check is n_rows + 1"""
    from latok_amd import batch
    csr = cc.sparse_rows_case()
    indptr, indices, data = csr
    n_rows = indptr.size - 1
    broken = indptr.copy()
    broken[n_rows - 1] = 6                                                                   # 6 > 5 = indptr[n_rows]
    for dt in (np.int64, np.int32):
        with batch.Idf(cc.N_COLS) as f:
            f.update_csr(indptr.astype(dt), indices)
            assert np.array_equal(f.df(), np.bincount(indices, minlength=cc.N_COLS)) and f.n_docs == n_rows
            with pytest.raises(ValueError, match="non-decreasing"):
                f.update_csr(broken.astype(dt), indices)
            assert np.array_equal(f.df(), np.bincount(indices, minlength=cc.N_COLS)) and f.n_docs == n_rows
        with pytest.raises(ValueError, match="non-decreasing"):
            batch.tfidf_csr(broken.astype(dt), indices, data, idf)
    _report("more rows than entries", _sweep(csr, idf, idf_vec, cc.OPTS_FEW, "sparse rows"))


def test_idf_vector_of_more_than_a_million_columns(gpu):
    """2^20 + 3 columns: k_idf_weights strides twice over its 2048 x 256 threads; the whole vector, both smoothing modes"""
    from latok_amd import batch
    n_cols = 2 ** 20 + 3
    assert n_cols > 2 * cc.STRIDE_LIMIT
    df, n_docs = cc.fixed_df(n_cols, seed=6, n_docs=2 ** 31 - 1000)
    df[-1], df[-2], df[cc.STRIDE_LIMIT], df[cc.STRIDE_LIMIT - 1] = n_docs, 0, 1, 0
    with batch.Idf(n_cols) as f:
        f.load(df, n_docs)
        assert np.array_equal(f.df(), df) and f.n_docs == n_docs
        for smooth in (True, False):
            got, exact = f.weights(smooth), ref.idf(df, n_docs, smooth)
            err = np.abs(got - exact).max() / (2.0 ** -24 * np.abs(exact).max())
            _report("idf vector of 2^20 + 3 columns, smooth=%s" % smooth, err)
            assert err <= 1 and ((got == 0) == (exact == 0)).all() and np.isfinite(got).all()


# ---- 10: unsorted and repeated columns -------------------------------------------------------------------------------
def test_repeated_columns(idf, idf_vec, gpu):
    """the header: latok_idf_update_csr "does not check that" columns are distinct -- every stored entry counts; the weighting goes entry
    by entry"""
    from latok_amd import batch
    S, W, SLOTS = cc.limits()
    csr = cc.repeated_columns_case(S, W)
    for a, b in zip(csr[0][:-1], csr[0][1:]):
        assert np.unique(csr[1][a:b]).size < b - a and (b - a < 5 or (np.diff(csr[1][a:b]) < 0).any())
    with batch.Idf(cc.N_COLS) as f:
        f.update_csr(csr[0], csr[1])
        assert np.array_equal(f.df(), np.bincount(csr[1], minlength=cc.N_COLS)) and f.n_docs == csr[0].size - 1
    _report("repeated columns", _sweep(csr, idf, idf_vec, cc.OPTS, "repeated"))
