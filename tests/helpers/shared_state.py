"""Which state of a shared, mutable object did a call see?  The judge of tests/test_gpu_shared_objects.py, kept apart from the GPU so
that tests/test_shared_objects_host.py can show what it accepts and what it refuses.

An idf that an updater thread takes through states 0 .. J (state j = after j updates) is transformed meanwhile by reader threads.  The
lock inside the object promises that every call sees ONE whole state.  The test computes the J + 1 expected outputs beforehand
(tests/helpers/tfidf_ref.py, float64) and every observed output then has to lie within the error bound of the header (tfidf_ref.worst)
of exactly one of them -- as a whole: an output whose rows come from two states matches none.  That verdict means something only if
the states are far apart on the scale of the bound, which is a property of the reference alone and is asserted before any device work:

  separation(expected, indptr, norm)   for every row and every pair of states the row's largest entry distance, in units of the
                                       entry's bound; the smallest of them with its (state, state, row)
  assert_separable(...)                that margin is at least SEPARATION = 64
  match_state(observed, ...)           the one state whose bound holds the output, else AssertionError
  vector_separation / match_vector     the same for an idf vector, held to 2^-24 of its largest weight (tests/test_gpu_tfidf.py)
  StateCorpus, rows_csr                the corpus of that test in column ids, with df, n_docs and the expected outputs of every state
  check_order(states)                  a reader's states never go backwards
  check_window(state, lo, hi)          a call that began after update lo returned and ended before update hi + 1 began saw lo .. hi"""
import numpy as np

from helpers import tfidf_ref as ref

SEPARATION = 64.0
VECTOR_REL = 2.0 ** -24


def separation(expected_by_state, indptr, norm):
    """(margin, (i, j, row)): the smallest, over every row and every pair of states i < j, of the row's largest |a - b| / (bound *
    max(|a|, |b|)).  A row without entries separates nothing: margin 0."""
    indptr = np.asarray(indptr, np.int64)
    exp = [np.asarray(e, np.float64) for e in expected_by_state]
    assert len(exp) >= 2 and all(e.shape == (int(indptr[-1]),) for e in exp), "one expected output of nnz entries per state"
    b = ref.bounds(indptr, norm)
    best, where = np.inf, None
    for i in range(len(exp)):
        for j in range(i + 1, len(exp)):
            scale = np.maximum(np.abs(exp[i]), np.abs(exp[j])) * b
            dist = np.where(scale > 0, np.abs(exp[i] - exp[j]) / np.where(scale > 0, scale, 1.0), 0.0)
            for r in range(indptr.size - 1):
                a, e = int(indptr[r]), int(indptr[r + 1])
                m = float(dist[a:e].max()) if e > a else 0.0
                if m < best:
                    best, where = m, (i, j, r)
    return best, where


def assert_separable(expected_by_state, indptr, norm, factor=SEPARATION):
    margin, where = separation(expected_by_state, indptr, norm)
    assert margin >= factor, "states %d and %d differ by only %.3g bounds in row %d (norm=%r): the corpus cannot tell them apart" % (
        where[0], where[1], margin, where[2], norm)
    return margin


def _one(hits, report):
    if len(hits) != 1:
        raise AssertionError("the output lies within the bound of %s; %s" % ("no state" if not hits else "states %r" % (hits,), report))
    return hits[0]


def match_state(observed, expected_by_state, indptr, norm):
    """the index of the one state whose bound holds every entry of ``observed``; AssertionError for none (a wrong or torn output) or
    several (states that were not separable)"""
    observed = np.asarray(observed)
    ratios = []
    for exp in expected_by_state:
        if observed.shape != np.asarray(exp).shape:
            raise AssertionError("the output has %r entries, the reference %r" % (observed.shape, np.asarray(exp).shape))
        ratios.append(ref.worst(observed, exp, indptr, norm)[0])
    hits = [j for j, w in enumerate(ratios) if w <= 1]
    if len(hits) == 1:
        return hits[0]
    # for the message: the nearest state of every row on its own (a torn output shows as rows that disagree)
    indptr = np.asarray(indptr, np.int64)
    rows = []
    for r in range(indptr.size - 1):
        a, e = int(indptr[r]), int(indptr[r + 1])
        if e > a:
            per = [ref.worst(observed[a:e], np.asarray(exp)[a:e], [0, e - a], norm)[0] for exp in expected_by_state]
            rows.append(int(np.argmin(per)))
    return _one(hits, "worst error over the bound per state %s; nearest state of every row %s" % (["%.3g" % w for w in ratios], rows))


def _vector_within(got, exact, rel):
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    return bool(np.isfinite(got).all() and ((got == 0) == (exact == 0)).all() and np.abs(got - exact).max() <= rel * np.abs(exact).max())


def vector_separation(vectors_by_state, rel=VECTOR_REL):
    """the smallest distance of two states' vectors (largest entry difference), in units of rel * the larger of their largest weights"""
    vec = [np.asarray(v, np.float64) for v in vectors_by_state]
    assert len(vec) >= 2
    return min(float(np.abs(vec[i] - vec[j]).max() / (rel * max(np.abs(vec[i]).max(), np.abs(vec[j]).max())))
               for i in range(len(vec)) for j in range(i + 1, len(vec)))


def assert_vectors_separable(vectors_by_state, rel=VECTOR_REL, factor=SEPARATION):
    margin = vector_separation(vectors_by_state, rel)
    assert margin >= factor, "two states' idf vectors differ by only %.3g bounds" % margin
    return margin


def match_vector(observed, vectors_by_state, rel=VECTOR_REL):
    """match_state for an idf vector: within rel * max|exact| of exactly one state, zeros where that state has zeros"""
    observed = np.asarray(observed)
    for v in vectors_by_state:
        if observed.shape != np.asarray(v).shape:
            raise AssertionError("the vector has %r entries, the reference %r" % (observed.shape, np.asarray(v).shape))
    hits = [j for j, v in enumerate(vectors_by_state) if _vector_within(observed, v, rel)]
    return _one(hits, "largest distance per state %s" % ["%.3g" % float(np.abs(np.asarray(observed, np.float64) - np.asarray(v, np.float64)).max())
                                                        for v in vectors_by_state])


def rows_csr(docs):
    """lists of column ids (with repeats) -> (indptr int64, indices int32, data int32): the canonical CSR of their counts"""
    indptr, indices, data = [0], [], []
    for doc in docs:
        cols, cnt = np.unique(np.asarray(doc, np.int64), return_counts=True)
        indices += cols.tolist()
        data += cnt.tolist()
        indptr.append(len(indices))
    return np.asarray(indptr, np.int64), np.asarray(indices, np.int32), np.asarray(data, np.int32)


class StateCorpus:
    """The corpus of the "one whole state" test, in column ids (the GPU test spells column c as its c-th word).

    Columns 0 .. 15 are the PROBE columns.  ``base`` (n_base documents, the fit of state 0) holds probe column c in every (c + 2)-th
    document, so df[c] = ceil(n_base / (c + 2)): 20, 14, 10, 8, 7, 6, 5, 5, 4, ... for 40.  ``updates[j]`` has n_base * 2^j documents
    over columns 100 .. n_cols - 1 only (some of them empty), so after j updates n_docs = n_base * 2^j while df of the probe columns
    stands still.  ``probe`` rows hold one column of df >= 8, one of df 4 .. 7 and one of df 3, each one to three times: three different
    df in every row, so an L2 row moves with n_docs as well."""

    PROBE_COLS, UPDATE_LO = 16, 100

    def __init__(self, n_updates=6, n_base=40, n_cols=1000, n_probe=10, seed=7):
        rng = np.random.default_rng(seed)
        self.n_cols, self.n_updates = n_cols, n_updates
        self.base = [[c for c in range(self.PROBE_COLS) if d % (c + 2) == 0] for d in range(n_base)]
        self.probe = []
        for r in range(n_probe):
            row = [r % 4] * (1 + r % 3) + [4 + r % 5] * (1 + (r + 1) % 3) + [12 + r % 4] * (1 + (r + 2) % 3)
            self.probe.append([row[i] for i in rng.permutation(len(row))])
        self.updates = []
        for j in range(n_updates):
            docs = [rng.integers(self.UPDATE_LO, n_cols, int(k)).tolist() for k in rng.integers(0, 6, n_base << j)]
            self.updates.append(docs)
        self.df, self.n_docs = [], []
        df = ref.document_frequency(rows_csr(self.base)[1], n_cols)
        n = len(self.base)
        for j in range(n_updates + 1):
            self.df.append(df.copy())
            self.n_docs.append(n)
            if j < n_updates:
                df = df + ref.document_frequency(rows_csr(self.updates[j])[1], n_cols)
                n += len(self.updates[j])
        self.csr = rows_csr(self.probe)

    def idf_vectors(self, smooth):
        """float64[n_cols] per state"""
        return [ref.idf(df, n, smooth) for df, n in zip(self.df, self.n_docs)]

    def expected(self, smooth, norm, sublinear_tf=False):
        """float64[nnz] per state: the probe rows' weighting"""
        indptr, indices, data = self.csr
        return [ref.weigh(indptr, indices, data, v, sublinear_tf, norm) for v in self.idf_vectors(smooth)]


def check_order(states):
    """the states one reader saw, in the order of its calls: never backwards"""
    states = [int(s) for s in states]
    for k in range(1, len(states)):
        assert states[k] >= states[k - 1], "call %d saw state %d after call %d saw state %d: %r" % (k, states[k], k - 1, states[k - 1], states)
    return states


def check_window(state, lo, hi):
    """``lo`` updates had returned before the call began and ``hi`` had begun when it ended: the call saw one of lo .. hi"""
    assert lo <= state <= hi, "a call saw state %d, but %d updates had returned before it began and %d had begun when it ended" % (state, lo, hi)
    return state
