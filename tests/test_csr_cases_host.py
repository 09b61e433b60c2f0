"""tests/helpers/csr_cases.py without a device: the builder gives valid CSRs of the stated lengths and kinds; its vectorised weigh()
equals tfidf_ref.weigh bit for bit on every small case; a spike row's outputs move by more than 100 bounds when the spike is left out
of the norm or counted twice; the colliding columns of the k_df_add case share an LDS slot and the others do not; and every value the
device tests expect is finite and, where it is not zero, a normal float32 -- so "exactly zero where the rule says zero" cannot be
confused with underflow."""
import numpy as np
import pytest

from helpers import csr_cases as cc
from helpers import tfidf_ref as ref


@pytest.fixture(scope="module")
def lim():
    return cc.limits()


@pytest.fixture(scope="module")
def cases(lim):
    return list(cc.weigh_cases(lim[0], lim[1]))


def _valid(indptr, indices, data, n_cols=cc.N_COLS):
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.int32
    assert indptr[0] == 0 and (np.diff(indptr) >= 0).all() and indptr[-1] == indices.size == data.size
    assert indices.size == 0 or (0 <= indices.min() and indices.max() < n_cols)


def _rows(csr):
    indptr, indices, data = csr
    return [(indices[a:b], data[a:b]) for a, b in zip(indptr[:-1], indptr[1:])]


def test_builder_lengths_kinds_and_columns(lim):
    S, W, _ = lim
    lens = [0, 1, 17, S, S + 1, W, W + 1, 5 * W + 3]
    for kind in cc.KINDS + (cc.spike(0),):
        csr = cc.build([(k, kind) for k in lens if k > 0 or kind in cc.KINDS], seed=3)
        _valid(*csr)
        assert np.diff(csr[0]).tolist() == [k for k in lens if k > 0 or kind in cc.KINDS]
        for cols, data in _rows(csr):
            assert np.unique(cols).size == cols.size                                   # distinct within the row
            if kind == "small":
                assert data.size == 0 or (1 <= data.min() and data.max() <= 49)
            elif kind == "signed":
                assert data.size == 0 or (-50 <= data.min() and data.max() <= 49)
                assert data.size < 3 or (data == 0).any()
            elif kind == "extreme":
                assert set(data.tolist()) <= set(cc.EXTREME)
            elif kind == "zeros":
                assert not data.any()
            else:
                assert data[0] == cc.SPIKE and (data[1:] == 1).all()
        long_rows = [cols for cols, _ in _rows(csr) if cols.size > 64]
        assert all((np.diff(cols) < 0).any() for cols in long_rows)                    # not sorted
    big = cc.build([(5 * W + 3, "extreme")], seed=4)[2]
    assert set(big.tolist()) == set(cc.EXTREME)                                        # a long row meets every extreme value
    a, b = cc.build([(40, "signed"), (90, "small")], seed=9), cc.build([(40, "signed"), (90, "small")], seed=9)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))                             # a fixed seed: the same CSR every time
    with pytest.raises(ValueError):
        cc.build([(4, cc.spike(4))])
    made = cc.row(5, "small", np.random.default_rng(1))
    again = cc.build([(3, "small"), made, (0, "zeros")])
    assert np.array_equal(again[1][3:8], made[0]) and np.array_equal(again[2][3:8], made[1]) and again[0].tolist() == [0, 3, 8, 8]
    over = cc.build([(40 * W + 5, "small")], seed=2)                                   # longer than N_COLS: permutation after permutation
    _valid(*over)
    assert all(np.unique(over[1][i:i + cc.N_COLS]).size == min(cc.N_COLS, over[1].size - i) for i in range(0, over[1].size, cc.N_COLS))


def test_layouts_put_the_long_rows_where_they_say(lim):
    S, W, _ = lim
    lay = cc.long_row_layouts(S, W)
    starts = {}
    for name, lens in lay.items():
        indptr = np.concatenate([[0], np.cumsum(lens)])
        starts[name] = [(int(indptr[i]), k) for i, k in enumerate(lens) if k > W]
        assert starts[name], name
        tiles = [s // W for s, _ in starts[name]]
        assert len(set(tiles)) == len(tiles), name                                     # at most one long row starts in a tile
        _valid(*cc.long_row_case(name, S, W))
    assert cc.long_starts(S, W) == [0, W - 1, W, W + 1, 2 * W - 1]
    for (a, _), start in zip(cc._STARTS, cc.long_starts(S, W)):
        for (b, _), k in zip(cc._LENGTHS, cc.long_lengths(S, W)):
            name = "start_%s_len_%s" % (a, b)
            assert starts[name] == [(start, k)]
            front = lay[name][:-2]
            assert all(f <= W for f in front) and (start < W or W in front) and (start < 100 or any(S < f <= W for f in front))
    assert cc.long_lengths(S, W) == [W + 1, 2 * W, 2 * W + 1, 5 * W + 3, 40 * W + 5]
    assert [s // W for s, _ in starts["two_back_to_back"]] == [0, 1] and [s // W for s, _ in starts["three_back_to_back"]] == [0, 1, 2]
    assert [s for s, _ in starts["three_back_to_back_from_tile_end"]] == [W - 1, 2 * W, 4 * W]
    assert lay["behind_three_empty_rows"][1:4] == [0, 0, 0] and lay["behind_three_empty_rows"][4] > W
    assert starts["behind_three_empty_rows_at_tile_start"] == [(W, 2 * W + 1)]
    assert lay["before_three_trailing_empty_rows"][-3:] == [0, 0, 0] and lay["before_three_trailing_empty_rows"][-4] > W
    for name, rem, n in (("only_row_nnz_multiple", 0, 1), ("only_row_nnz_multiple_plus_1", 1, 1), ("last_row_nnz_multiple", 0, 2),
                         ("last_row_nnz_multiple_plus_1", 1, 2)):
        assert len(lay[name]) == n and lay[name][-1] > W and sum(lay[name]) % W == rem
    wave = cc.wave_layouts(S, W)
    assert sorted({len(v) for k, v in wave.items() if "_rows" in k}) == [1, 3, 15, 16, 17]
    assert set(cc.wave_groups(S, W).values()) == {(0, S, S + 1, W), (W, W, W, W), (W + 1, 0, 1, S + 1), (S + 1, S + 1, W, 0)}
    for e in (1, 15, 16, 17, S - 1, S, S + 1):                                         # every edge length in every place of a wave
        assert {i % 4 for k, v in wave.items() if k.startswith("lane_edges") for i, x in enumerate(v) if x == e} == {0, 1, 2, 3}
    rows = cc.independence_rows(S, W)
    assert [r[0].size for r in rows] == [1, S, S + 1, W, W + 1, 2 * W + 1, 5 * W + 3]
    seen = [set() for _ in rows]
    for b in (1, 2, 3):
        csr, where = cc.independence_batch(rows, b, S, W)
        _valid(*csr)
        for i, (w, r) in enumerate(zip(where, rows)):
            a = int(csr[0][w])
            assert np.array_equal(csr[1][a:a + r[0].size], r[0]) and np.array_equal(csr[2][a:a + r[1].size], r[1]) and a % 4 == b
            seen[i].add((a % W) < W // 2)
    assert all(s == {False, True} for s, r in zip(seen, rows) if r[0].size > S)        # below and above a tile edge
    ks = [k for k, _ in cc.spike_rows(S, W)]
    assert sorted(set(ks)) == [S + 1, W, W + 1, 2 * W + 1, 5 * W + 3]
    assert {p for k, p in cc.spike_rows(S, W) if k == 2 * W + 1} == {0, 15, 16, 63, 64, 255, 256, W - 1, W, W + 1, 2 * W + 1 - 257, 2 * W + 1 - 256,
                                                                     2 * W - 1, 2 * W}
    indptr, indices, data = cc.spike_case(S, W)
    for (k, p), a in zip(cc.spike_rows(S, W), indptr[:-1]):
        assert data[a + p] == cc.SPIKE and data[a:a + k].sum() == k - 1 + cc.SPIKE


def test_vectorised_weigh_equals_the_reference(lim, cases):
    df, n_docs = cc.fixed_df()
    n = 0
    for name, csr, with_idf in cases:
        if csr[0].size > 5000:
            continue
        for smooth, sub, norm in cc.OPTS:
            vec = ref.idf(df, n_docs, smooth) if with_idf else None
            a, b = ref.weigh(*csr, vec, sub, norm), cc.weigh(*csr, vec, sub, norm)
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (name, smooth, sub, norm)
        n += 1
    assert n >= len(cases) - 1
    empty = (np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert cc.weigh(*empty).size == 0 and ref.weigh(*empty).size == 0
    one = cc.stride_case(n_rows=cc.STRIDE_LIMIT // 64)                                 # the large case's own shape, cut down
    for norm in ("l2", "l1", None):
        assert np.array_equal(ref.weigh(*one, ref.idf(df, n_docs, True), True, norm), cc.weigh(*one, ref.idf(df, n_docs, True), True, norm))


def test_a_wrong_spike_term_moves_a_row_by_more_than_100_bounds(lim):
    """in the float64 reference alone: the norm without the spike's term, or with it twice, against the right one"""
    S, W, _ = lim
    indptr, indices, data = cc.spike_case(S, W)
    for norm in ("l2", "l1"):
        want = ref.weigh(indptr, indices, data, None, False, norm)
        for r, (k, p) in enumerate(cc.spike_rows(S, W)):
            a, b = int(indptr[r]), int(indptr[r + 1])
            w = data[a:b].astype(np.float64)
            terms = w ** 2 if norm == "l2" else np.abs(w)
            bound = (k + 16) * ref.EPS
            for factor in (0.0, 2.0):
                t = terms.copy()
                t[p] *= factor
                wrong = w / (np.sqrt(t.sum()) if norm == "l2" else t.sum())
                move = np.abs(wrong - want[a:b]) / np.abs(want[a:b])
                assert move.min() > 100 * bound, (norm, k, p, factor, move.min() / bound)
            removed, doubled = cc.spike_shift(k, norm)
            assert min(removed, doubled) > 100


def test_colliding_columns_share_a_slot(lim):
    _, _, slots = lim
    assert cc.slot(1, 1024) == cc.slot(1450, 1024) == cc.slot(2013, 1024)
    assert cc.colliding_columns(1024) == [1, 1450, 2013]
    assert int(cc.slot(3, 1024)) == ((3 * 2654435761 % 2 ** 32) >> 16) % 1024 and int(cc.slot(2 ** 31 - 1, 1024)) < 1024
    indptr, indices, n_cols, (a, b), own = cc.df_collision_case(slots)
    assert a != b and cc.slot(a, slots) == cc.slot(b, slots)
    assert (cc.slot(own, slots) != cc.slot(a, slots)).all() and np.unique(own).size == own.size
    assert indices.size == 3 * cc.DF_CHUNK + 5 and indptr[-1] == indices.size and (np.diff(indptr)[:-1] == 3).all() and np.diff(indptr)[-1] == 2
    assert indices[-2] == 0 and indices[-1] == n_cols - 1 and 0 not in own and n_cols - 1 not in own
    count = np.bincount(indices, minlength=n_cols)
    assert count[a] == count[b] == own.size and (count[own] == 1).all() and count[0] == 1 and count[n_cols - 1] == 1
    for chunk in range(0, indices.size, cc.DF_CHUNK):                                  # every workgroup of k_df_add meets both hot columns
        part = indices[chunk:chunk + cc.DF_CHUNK]
        assert (part == a).any() and (part == b).any()


def test_large_cases_are_what_they_claim(lim):
    indptr, indices, data = cc.stride_case()
    _valid(indptr, indices, data)
    assert indptr.size - 1 == indices.size == 600001 and data[-1] != 0
    for name, (ip, ix, words) in cc.stride_defects(indptr, indices, cc.N_COLS).items():
        bad_order = (np.diff(ip) < 0).nonzero()[0]
        bad_col = ((ix < 0) | (ix >= cc.N_COLS)).nonzero()[0]
        assert (bad_order.size, bad_col.size, int(ip[-1] != ix.size)) in ((1, 0, 0), (0, 1, 0), (0, 0, 1)), name   # one defect
        assert all(i > cc.STRIDE_LIMIT for i in np.concatenate([bad_order, bad_col])), name
        assert words == ("non-decreasing" if bad_order.size else "column" if bad_col.size else "does not match nnz")
    ip, ix, d = cc.sparse_rows_case()
    _valid(ip, ix, d)
    assert ip.size - 1 == 600000 and ix.size == 5 and ip.size > cc.STRIDE_LIMIT and np.diff(ip).max() == 2 and ip[-2] == 5


def test_every_expected_value_is_finite_and_normal(lim, cases):
    df, n_docs = cc.fixed_df()
    assert (df == 0).any() and (df == n_docs).any() and df.max() <= n_docs
    for name, csr, with_idf in cases:
        _valid(*csr)
        for smooth, sub, norm in cc.OPTS:
            vec = ref.idf(df, n_docs, smooth) if with_idf else None
            want = cc.weigh(*csr, vec, sub, norm)
            assert np.isfinite(want).all(), (name, smooth, sub, norm)
            nz = want != 0
            assert (np.abs(want[nz]) > cc.F32_MIN_NORMAL).all() and (np.abs(want[nz]) < 2.0 ** 127).all(), (name, smooth, sub, norm)
            zero = (csr[2] == 0) | ((vec[csr[1]] == 0) if vec is not None else False)  # the rule's zeros: a zero count, a zero idf
            assert np.array_equal(~nz, zero | ~nz) and (want[zero] == 0).all() and np.array_equal(nz, ~zero), (name, smooth, sub, norm)
