"""The TF-IDF rules of latok_idf_* and latok_tfidf_csr (include/latok_hip.h) in numpy float64, written from their statement and not
from the C++ header:

  df[c]   = number of stored entries with column c (explicit zeros count): np.bincount(indices, minlength=n_cols)
  idf[c]  = ln((n + s) / (df[c] + s)) + 1, s = 1 if smooth else 0; without smoothing df[c] = 0 gives 0
  tf      = t, or with sublinear tf: sign(t) * (1 + ln|t|) for t != 0 and 0 for t = 0
  w       = tf * idf[c] (tf without an idf);  out = w / N_r with N_r = sqrt(sum w^2) (l2), sum |w| (l1), 1 (None)
  a row whose norm is 0 keeps its zeros

and the error bounds a float32 result is held to: (k + 16) * 2^-23 relative for a normalised row of k stored entries, 8 * 2^-23 without a
norm, exact zeros where the rule says zero."""
import numpy as np

EPS = 2.0 ** -23


def document_frequency(indices, n_cols):
    return np.bincount(np.asarray(indices, np.int64), minlength=n_cols).astype(np.int64)


def idf(df, n_docs, smooth):
    df = np.asarray(df, np.float64)
    s = 1.0 if smooth else 0.0
    out = np.zeros(df.shape, np.float64)
    ok = (df + s) > 0
    out[ok] = np.log((float(n_docs) + s) / (df[ok] + s)) + 1.0
    return out


def tf(t, sublinear):
    t = np.asarray(t, np.float64)
    if not sublinear:
        return t.copy()
    out = np.zeros(t.shape, np.float64)
    nz = t != 0
    out[nz] = np.sign(t[nz]) * (1.0 + np.log(np.abs(t[nz])))
    return out


def weigh(indptr, indices, data, idf_vec=None, sublinear_tf=False, norm="l2"):
    """float64[nnz]: the weighting of the CSR"""
    indptr = np.asarray(indptr, np.int64)
    w = tf(data, sublinear_tf)
    if idf_vec is not None:
        w = w * np.asarray(idf_vec, np.float64)[np.asarray(indices, np.int64)]
    out = w.copy()
    if norm is None:
        return out
    for r in range(indptr.size - 1):
        a, b = indptr[r], indptr[r + 1]
        n = np.sqrt(np.sum(w[a:b] ** 2)) if norm == "l2" else np.sum(np.abs(w[a:b]))
        if n > 0:
            out[a:b] = w[a:b] / n
    return out


def bounds(indptr, norm):
    """the relative error bound of every entry"""
    indptr = np.asarray(indptr, np.int64)
    k = np.repeat(np.diff(indptr), np.diff(indptr)).astype(np.float64)
    return (k + 16.0) * EPS if norm is not None else np.full(k.shape, 8.0 * EPS)


def worst(got, want, indptr, norm):
    """(worst error over its bound, index): <= 1 passes.  Where the reference is 0 the result has to be exactly 0; NaN and infinity
    never pass."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.size == 0:
        return 0.0, -1
    b = bounds(indptr, norm)
    ratio = np.where(want == 0, np.where(got == 0, 0.0, np.inf), np.abs(got - want) / (np.abs(want) * b + (want == 0)))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    i = int(np.argmax(ratio))
    return float(ratio[i]), i
