"""Caller-built CSRs for latok_tfidf_csr and latok_idf_update_csr (include/latok_hip.h): what the library's own count kernels never
write.  Rows are built from a list of lengths; their columns are distinct within a row (while the row is no longer than N_COLS: a
longer one walks through fresh permutations), NOT sorted, and drawn from N_COLS columns with a fixed seed; their data comes from one
named kind:

  small     1 .. 49
  signed    -50 .. 49, zeros included
  extreme   drawn from INT32_MIN, INT32_MAX, 2^24 + 1 (where int32 -> float32 rounds), 1, -1, 0, 7
  zeros     all 0
  spike(p)  all 1 except entry p, which is 1000: a kernel that skips or repeats entry p in the norm moves every output of the row far
            beyond the header's bound (spike_shift), which a row of equal entries would hide

The layouts below place rows at the positions where tfidf_kernels.hip takes another path; S = kTfidfSubMax, W = kTfidfWaveMax and
kDfSlots are read from the library (limits()), never written down here.  weigh() is tfidf_ref.weigh without the loop over rows, for
CSRs of many rows.  Both the device tests (test_gpu_tfidf_csr.py) and the host test (test_csr_cases_host.py) take their cases from
here, so what the host test proves about the expected values holds for what the device is asked."""
import ctypes as C
import functools
import itertools

import numpy as np

from helpers import tfidf_ref as ref

N_COLS = 8192
DF_CHUNK = 16384                  # kDfChunk (tfidf_kernels.hip): the entries one workgroup of k_df_add takes
STRIDE_LIMIT = 2048 * 256         # stride_grid() (tfidf_kernels.hip): k_csr_check and k_idf_weights launch at most 2048 x 256 threads
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
BIG = 2 ** 24 + 1                 # the first int32 that float32 cannot hold
EXTREME = (I32_MIN, I32_MAX, BIG, 1, -1, 0, 7)
KINDS = ("small", "signed", "extreme", "zeros")
SPIKE = 1000
F32_MIN_NORMAL = 2.0 ** -126
OPTS = list(itertools.product((False, True), (False, True), ("l1", "l2", None)))   # smooth_idf, sublinear_tf, norm
OPTS_FEW = [(True, False, "l2"), (False, True, "l1"), (False, False, None)]       # the least a case is run with


@functools.lru_cache(maxsize=1)
def limits():
    """(kTfidfSubMax, kTfidfWaveMax, kDfSlots) of the built library; needs no device"""
    from latok_amd import _lib
    lib = _lib.load()
    out = (C.c_int64 * 3)()
    assert lib.latok_debug_tfidf_limits(out, 3) == 3
    sub, wave, slots = (int(v) for v in out)
    assert 16 <= sub and sub + 1 < wave and 5 * wave + 3 < N_COLS and slots & (slots - 1) == 0
    return sub, wave, slots


def slot(c, slots):
    """the LDS slot of column c in k_df_add: ((c * 2654435761 mod 2^32) >> 16) & (kDfSlots - 1)"""
    c = np.asarray(c, np.uint64)
    return (((c * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(16)) & np.uint64(slots - 1)


def spike(p):
    return ("spike", int(p))


def row(k, kind, rng):
    """(indices int32[k], data int32[k]) of one row"""
    cols = np.concatenate([rng.permutation(N_COLS) for _ in range(-(-k // N_COLS))] or [np.zeros(0, np.int64)])[:k]
    if kind == "small":
        data = rng.integers(1, 50, k)
    elif kind == "signed":
        data = rng.integers(-50, 50, k)
        if k >= 3:
            data[rng.integers(0, k)] = 0
    elif kind == "extreme":
        data = np.asarray(EXTREME, np.int64)[rng.integers(0, len(EXTREME), k)]
    elif kind == "zeros":
        data = np.zeros(k, np.int64)
    elif isinstance(kind, tuple) and kind[0] == "spike" and 0 <= kind[1] < k:
        data = np.ones(k, np.int64)
        data[kind[1]] = SPIKE
    else:
        raise ValueError("unknown kind %r for a row of %d" % (kind, k))
    return cols.astype(np.int32), data.astype(np.int32)


def build(rows, seed=0):
    """rows: (length, kind) pairs, or (indices, data) arrays of a row made before -> (indptr int64, indices int32, data int32)"""
    rng = np.random.default_rng(seed)
    made = [r if isinstance(r[0], np.ndarray) else row(int(r[0]), r[1], rng) for r in rows]
    indptr = np.zeros(len(made) + 1, np.int64)
    np.cumsum([m[0].size for m in made], out=indptr[1:])
    cat = lambda i, dt: np.concatenate([m[i] for m in made]).astype(dt) if made else np.zeros(0, dt)
    return indptr, cat(0, np.int32), cat(1, np.int32)


def weigh(indptr, indices, data, idf_vec=None, sublinear_tf=False, norm="l2"):
    """tfidf_ref.weigh, float64[nnz], bit for bit: one np.sum over all rows of one length in place of the loop over rows"""
    indptr = np.asarray(indptr, np.int64)
    w = ref.tf(data, sublinear_tf)
    if idf_vec is not None:
        w = w * np.asarray(idf_vec, np.float64)[np.asarray(indices, np.int64)]
    out = w.copy()
    lens = np.diff(indptr)
    if norm is None or w.size == 0:
        return out
    terms, sums = (w ** 2 if norm == "l2" else np.abs(w)), np.zeros(lens.size, np.float64)
    for k in np.unique(lens[lens > 0]):                                 # (np.add.reduceat adds in another order than np.sum does)
        rows = np.nonzero(lens == k)[0]
        sums[rows] = np.sum(terms[indptr[rows][:, None] + np.arange(k)], axis=1)
    n = np.repeat(np.sqrt(sums) if norm == "l2" else sums, lens)
    ok = n > 0
    out[ok] = w[ok] / n[ok]
    return out


def fixed_df(n_cols=N_COLS, seed=5, n_docs=1000):
    """(df int32[n_cols], n_docs): random, with columns that no document holds and columns that every document holds"""
    rng = np.random.default_rng(seed)
    df = rng.integers(1, n_docs + 1, n_cols)
    u = rng.random(n_cols)
    df[u < 0.1] = 0
    df[u > 0.97] = n_docs
    return df.astype(np.int32), n_docs


# ---- case 1: where a long row sits ----------------------------------------------------------------------------------
def _front(start, S, W):
    """short and wave-tier rows that hold `start` entries together, a row of exactly W entries among them where it fits"""
    rows, rem = [], start
    if rem >= W:
        rows.append(W)
        rem -= W
    for k in (17, S + 1):
        if rem > 0:
            rows.append(min(rem, k))
            rem -= rows[-1]
    while rem > 0:
        rows.append(min(rem, W))
        rem -= rows[-1]
    return rows


_STARTS = (("0", lambda W: 0), ("W-1", lambda W: W - 1), ("W", lambda W: W), ("W+1", lambda W: W + 1), ("2W-1", lambda W: 2 * W - 1))
_LENGTHS = (("W+1", lambda W: W + 1), ("2W", lambda W: 2 * W), ("2W+1", lambda W: 2 * W + 1), ("5W+3", lambda W: 5 * W + 3),
            ("40W+5", lambda W: 40 * W + 5))
LONG_ROW_NAMES = ["start_%s_len_%s" % (a, b) for a, _ in _STARTS for b, _ in _LENGTHS] + [
    "two_back_to_back", "three_back_to_back", "three_back_to_back_from_tile_end", "behind_three_empty_rows",
    "behind_three_empty_rows_at_tile_start", "before_three_trailing_empty_rows", "only_row_nnz_multiple", "only_row_nnz_multiple_plus_1",
    "last_row_nnz_multiple", "last_row_nnz_multiple_plus_1"]


def long_starts(S, W):
    return [f(W) for _, f in _STARTS]


def long_lengths(S, W):
    return [f(W) for _, f in _LENGTHS]


def long_row_layouts(S, W):
    """name -> row lengths.  A long row is taken by the workgroup of the tile of W entries in which it starts."""
    out = {}
    for a, start in _STARTS:
        for b, k in _LENGTHS:
            out["start_%s_len_%s" % (a, b)] = _front(start(W), S, W) + [k(W), 3]
    out["two_back_to_back"] = [W + 1, W + 1, 2]                        # starts 0 and W + 1: tiles 0 and 1
    out["three_back_to_back"] = [W + 1, W + 1, W + 1]                  # tiles 0, 1 and 2
    out["three_back_to_back_from_tile_end"] = _front(W - 1, S, W) + [W + 1, 2 * W, W + 2, 1]   # starts W - 1, 2W, 4W: tiles 0, 2, 4
    out["behind_three_empty_rows"] = [5, 0, 0, 0, W + 7, 3]
    out["behind_three_empty_rows_at_tile_start"] = [W, 0, 0, 0, 2 * W + 1]
    out["before_three_trailing_empty_rows"] = [5, 2 * W + 1, 0, 0, 0]
    out["only_row_nnz_multiple"] = [2 * W]
    out["only_row_nnz_multiple_plus_1"] = [2 * W + 1]
    out["last_row_nnz_multiple"] = [7, 2 * W - 7]
    out["last_row_nnz_multiple_plus_1"] = [7, 2 * W - 6]
    assert list(out) == LONG_ROW_NAMES
    return out


def long_row_case(name, S, W):
    lens = long_row_layouts(S, W)[name]
    kinds = itertools.cycle(("small", "signed"))
    return build([(k, "small" if k > W else next(kinds)) for k in lens], seed=11)


# ---- case 2: the tiers inside one wave ------------------------------------------------------------------------------
def wave_groups(S, W):
    return {"empty_sub_wave_wave": (0, S, S + 1, W), "four_wave_rows": (W, W, W, W), "long_empty_one_wave": (W + 1, 0, 1, S + 1),
            "wave_wave_wave_empty": (S + 1, S + 1, W, 0)}


WAVE_GROUP_NAMES = ("empty_sub_wave_wave", "four_wave_rows", "long_empty_one_wave", "wave_wave_wave_empty")
WAVE_NAMES = ["%s_%d_rows" % (g, n) for g in WAVE_GROUP_NAMES for n in (1, 3, 15, 16, 17)] + ["lane_edges_shift%d" % i for i in range(4)]


def wave_layouts(S, W):
    out = {}
    for name, g in wave_groups(S, W).items():
        for n_rows in (1, 3, 15, 16, 17):
            out["%s_%d_rows" % (name, n_rows)] = (list(g) * 5)[:n_rows]
    edges = [1, 15, 16, 17, S - 1, S, S + 1]
    for shift in range(4):                                              # every length in every one of a wave's four places
        out["lane_edges_shift%d" % shift] = [0] * shift + edges + [3] * ((-shift - len(edges)) % 4) + edges[::-1]
    assert list(out) == WAVE_NAMES
    return out


def wave_case(name, S, W):
    kinds = itertools.cycle(("small", "signed", "small", "extreme", "signed"))
    return build([(k, next(kinds)) for k in wave_layouts(S, W)[name]], seed=12)


# ---- case 3: every kind in every tier -------------------------------------------------------------------------------
def tier_lengths(S, W):
    return [1, 17, S, S + 1, W, W + 1, 2 * W + 1, 5 * W + 3]


def kind_case(kind, S, W):
    return build([(k, kind) for k in tier_lengths(S, W)], seed=13)


# ---- case 4: spike rows ---------------------------------------------------------------------------------------------
def spike_rows(S, W):
    """[(k, p)]: for every k one row per spike position"""
    out = []
    for k in (S + 1, W, W + 1, 2 * W + 1, 5 * W + 3):
        ps = {0, 15, 16, 63, 64, 255, 256, W - 1, W, W + 1, k - 257, k - 256, k - 2, k - 1}
        out += [(k, p) for p in sorted(ps) if 0 <= p < k]
    return out


def spike_case(S, W):
    return build([(k, spike(p)) for k, p in spike_rows(S, W)], seed=14)


def spike_shift(k, norm):
    """(removed, doubled): by how many bounds of a row of k entries every output moves when the spike's term is left out of the norm or
    added twice, in float64.  The outputs are w / N, so the relative move is N / N' - 1 for every entry alike."""
    term = float(SPIKE) ** 2 if norm == "l2" else float(SPIKE)
    rest = float(k - 1)
    root = np.sqrt if norm == "l2" else (lambda x: x)
    n = root(rest + term)
    bound = (k + 16.0) * ref.EPS
    return abs(n / root(rest) - 1.0) / bound, abs(n / root(rest + 2.0 * term) - 1.0) / bound


# ---- case 5: single-entry rows --------------------------------------------------------------------------------------
SINGLE_COUNTS = (1, -1, 2, -2, BIG, -BIG, I32_MAX, I32_MIN)


def single_entry_case(n_rows=4096, n_cols=N_COLS, seed=15):
    rng = np.random.default_rng(seed)
    data = np.asarray(SINGLE_COUNTS, np.int64)[rng.integers(0, len(SINGLE_COUNTS), n_rows)].astype(np.int32)
    data[:len(SINGLE_COUNTS)] = SINGLE_COUNTS
    indices = rng.integers(0, n_cols, n_rows).astype(np.int32)
    indices[:2] = 0, n_cols - 1
    return np.arange(n_rows + 1, dtype=np.int64), indices, data


# ---- case 6: a row's bits depend on the row alone -------------------------------------------------------------------
def independence_rows(S, W):
    """[(indices, data)] of the rows that are placed in several batches, each tier from another kind"""
    rng = np.random.default_rng(16)
    ks = [1, S, S + 1, W, W + 1, 2 * W + 1, 5 * W + 3]
    kinds = ["extreme", "signed", "small", spike(W // 2), "signed", "extreme", spike(5 * W)]
    return [row(k, kind, rng) for k, kind in zip(ks, kinds)]


def independence_batch(rows, b, S, W):
    """-> (csr, where): the rows behind fillers such that every row starts at an entry offset = b mod 4, and every row of more than S
    entries 4 - b entries below a tile edge (b = 1, 3) or b entries above it (b = 2); where[i] is the batch row of rows[i]"""
    assert b in (1, 2, 3) and W % 4 == 0
    items, where, cur = [], [], 0
    for r in rows:
        k = r[0].size
        target = cur + (b - cur) % 4
        if k > S:
            target = -(-(cur + 4) // W) * W + (b if b == 2 else b - 4)
        gap = target - cur
        if gap == 0:
            items.append((0, "small"))
        while gap > 0:
            items.append((min(gap, 1000), ("small", "signed")[len(items) % 2]))
            gap -= items[-1][0]
        where.append(len(items))
        items.append(r)
        cur = target + k
    csr = build(items + [(2, "small")], seed=17 + b)
    assert all(csr[0][w] % 4 == b for w in where)
    return csr, where


# ---- case 7: pointers -----------------------------------------------------------------------------------------------
def pointer_case(S, W):
    return build([(5, "signed"), (S + 1, "small"), (W, "signed"), (W + 1, "extreme"), (0, "small"), (17, "small"), (2 * W + 1, "signed")], seed=21)


# ---- case 8: latok_idf_update_csr, two hot columns in one LDS slot --------------------------------------------------
def colliding_columns(slots, n=3, limit=1 << 16):
    """the first n columns >= 1 that share the slot of column 1"""
    c = np.arange(1, limit)
    out = c[slot(c, slots) == slot(1, slots)][:n]
    assert out.size == n
    return [int(v) for v in out]


def df_collision_case(slots, n_cols=20000):
    """3 * DF_CHUNK + 5 entries: rows of (hot column a, hot column b, one column of the row's own) with a and b in one slot and every
    own column in another; the last row holds column 0 and column n_cols - 1"""
    n_rows = (3 * DF_CHUNK + 3) // 3
    a, b = colliding_columns(slots, 2)
    c = np.arange(1, n_cols - 1)
    own = c[(slot(c, slots) != slot(a, slots))][:n_rows]
    assert own.size == n_rows and a not in own and b not in own
    indices = np.empty(3 * n_rows + 2, np.int32)
    indices[0:3 * n_rows:3], indices[1:3 * n_rows:3], indices[2:3 * n_rows:3] = a, own, b
    indices[-2:] = 0, n_cols - 1
    indptr = np.concatenate([3 * np.arange(n_rows + 1), [3 * n_rows + 2]]).astype(np.int64)
    assert indices.size == 3 * DF_CHUNK + 5
    return indptr, indices, n_cols, (a, b), own


# ---- case 9: beyond the stride limit of k_csr_check and k_idf_weights -----------------------------------------------
def stride_case(n_rows=600001, n_cols=N_COLS, seed=19):
    rng = np.random.default_rng(seed)
    data = rng.integers(-50, 50, n_rows).astype(np.int32)
    data[-1] = 7
    return np.arange(n_rows + 1, dtype=np.int64), rng.integers(0, n_cols, n_rows).astype(np.int32), data


def stride_defects(indptr, indices, n_cols):
    """name -> (indptr, indices, the refusal's words): one defect each, all of them behind item STRIDE_LIMIT"""
    n_rows, nnz = indptr.size - 1, indices.size
    assert min(n_rows, nnz) - 1 > STRIDE_LIMIT

    def changed(a, i, v):
        a = a.copy()
        a[i] = v
        return a
    return {"column_n_cols_at_the_last_entry": (indptr, changed(indices, nnz - 1, n_cols), "column"),
            "column_minus_1_at_the_last_entry": (indptr, changed(indices, nnz - 1, -1), "column"),
            "indptr_descending_in_the_last_pair": (changed(indptr, n_rows - 1, nnz + 1), indices, "non-decreasing"),
            "indptr_ends_below_nnz": (changed(indptr, n_rows, nnz - 1), indices, "does not match nnz")}


def sparse_rows_case(n_rows=600000, n_cols=N_COLS):
    """n_rows + 1 > nnz: 5 entries in 600 000 rows"""
    indptr = np.zeros(n_rows + 1, np.int64)
    for r in (0, 1, 1, STRIDE_LIMIT + 1, n_rows - 2):                   # row 1 holds two entries
        indptr[r + 1:] += 1
    indices = np.array([3, 0, n_cols - 1, 3, 77], np.int32)
    assert indptr[-1] == 5 and indptr[-2] == 5
    return indptr, indices, np.array([2, -3, 1, 5, I32_MAX], np.int32)


# ---- case 10: unsorted and repeated columns -------------------------------------------------------------------------
def repeated_columns_case(S, W):
    rng = np.random.default_rng(20)
    rows = []
    for k in (2, 5, 17, S + 1, W + 1):
        cols = rng.integers(0, 9, k).astype(np.int32) * 1000            # at most 9 distinct columns: every row repeats some
        cols[-1] = cols[0]
        rows.append((cols, rng.integers(-5, 9, k).astype(np.int32)))
    return build(rows)


# ---- every weighting case, for the host test ------------------------------------------------------------------------
def weigh_cases(S, W):
    """(name, (indptr, indices, data), with_idf): every CSR that test_gpu_tfidf_csr.py hands to latok_tfidf_csr"""
    for name in long_row_layouts(S, W):
        yield "long:" + name, long_row_case(name, S, W), True
    for name in wave_layouts(S, W):
        yield "wave:" + name, wave_case(name, S, W), True
    for kind in KINDS:
        yield "kind:" + kind, kind_case(kind, S, W), True
    yield "spike", spike_case(S, W), False
    yield "single", single_entry_case(), True
    rows = independence_rows(S, W)
    yield "alone", build(rows), True
    for b in (1, 2, 3):
        yield "independence:%d" % b, independence_batch(rows, b, S, W)[0], True
    yield "pointers", pointer_case(S, W), True
    yield "stride", stride_case(), True
    yield "repeated", repeated_columns_case(S, W), True
