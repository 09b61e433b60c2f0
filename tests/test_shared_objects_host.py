"""The judge of tests/test_gpu_shared_objects.py (tests/helpers/shared_state.py) on the CPU: it names the right state for outputs the
reference made, and it refuses a torn output, an output beyond the bound, a sequence that goes backwards and a corpus whose states cannot
be told apart.  The corpus is the one the GPU test transforms, so its separability is established here as well.  And what the four handle
classes of latok_amd/batch.py share, without a device: close / with / __del__ over a library that only counts its destroy calls, the
handle lookup, and the packing of a word list."""
import itertools

import numpy as np
import pytest

from helpers import shared_state as ss
from helpers import tfidf_ref as ref

MODES = list(itertools.product((True, False), (None, "l2")))      # smooth_idf, norm: what the readers of the GPU test alternate


@pytest.fixture(scope="module")
def corpus():
    return ss.StateCorpus()


def _as_device(expected):
    """what a correct device call returns for a float64 reference: its float32 rounding (2^-24 relative, inside every bound)"""
    return np.asarray(expected, np.float64).astype(np.float32)


def test_the_corpus_is_what_the_gpu_test_needs(corpus):
    assert corpus.n_updates == 6 and len(corpus.df) == 7
    for j in range(6):
        assert corpus.n_docs[j + 1] == 2 * corpus.n_docs[j]                                        # every update doubles n_docs
        assert np.array_equal(corpus.df[j + 1][:ss.StateCorpus.UPDATE_LO], corpus.df[j][:ss.StateCorpus.UPDATE_LO])
        assert (corpus.df[j + 1] > corpus.df[j]).any()                                             # ... and really adds to df
        assert all(c >= ss.StateCorpus.UPDATE_LO for doc in corpus.updates[j] for c in doc) and [] in corpus.updates[j]
    indptr, indices, data = corpus.csr
    for r in range(len(corpus.probe)):
        cols = indices[indptr[r]:indptr[r + 1]]
        assert cols.max() < ss.StateCorpus.PROBE_COLS and len(set(corpus.df[0][cols].tolist())) >= 3   # three different df in every row
    assert data.max() == 3 and data.min() == 1


@pytest.mark.parametrize("smooth,norm", MODES)
def test_states_are_separable_and_the_reference_is_recognised(corpus, smooth, norm):
    indptr = corpus.csr[0]
    expected = corpus.expected(smooth, norm)
    margin = ss.assert_separable(expected, indptr, norm)
    assert margin >= 64
    print("separation of the probe rows, smooth=%r norm=%r: %.0f bounds" % (smooth, norm, margin))
    for j, e in enumerate(expected):
        assert ss.match_state(_as_device(e), expected, indptr, norm) == j
        assert ss.match_state(e, expected, indptr, norm) == j
    # an error of 0.9 bounds in every entry still names the state: the matcher asks no more than the header does
    j = 3
    inside = expected[j] * (1 + 0.9 * ref.bounds(indptr, norm) * np.where(np.arange(expected[j].size) % 2, 1, -1))
    assert ss.match_state(inside, expected, indptr, norm) == j


@pytest.mark.parametrize("smooth,norm", MODES)
def test_a_torn_output_matches_no_state(corpus, smooth, norm):
    indptr = corpus.csr[0]
    expected = corpus.expected(smooth, norm)
    for j in range(corpus.n_updates):
        for cut_row in (1, len(corpus.probe) // 2, len(corpus.probe) - 1):      # rows in front of cut_row from state j, the rest from j + 1
            torn = _as_device(expected[j]).copy()
            torn[indptr[cut_row]:] = _as_device(expected[j + 1])[indptr[cut_row]:]
            with pytest.raises(AssertionError, match="no state"):
                ss.match_state(torn, expected, indptr, norm)
    # one row of the next state is enough
    torn = _as_device(expected[2]).copy()
    torn[indptr[4]:indptr[5]] = _as_device(expected[3])[indptr[4]:indptr[5]]
    with pytest.raises(AssertionError, match="no state"):
        ss.match_state(torn, expected, indptr, norm)
    # ... and so is an idf vector that was half rewritten: weights of state j in front, of j + 1 behind
    vectors = corpus.idf_vectors(smooth)
    half = _as_device(vectors[1]).copy()
    half[corpus.n_cols // 2:] = _as_device(vectors[2])[corpus.n_cols // 2:]
    with pytest.raises(AssertionError, match="no state"):
        ss.match_vector(half, vectors)


@pytest.mark.parametrize("smooth,norm", MODES)
def test_an_output_beyond_the_bound_matches_no_state(corpus, smooth, norm):
    indptr = corpus.csr[0]
    expected = corpus.expected(smooth, norm)
    b = ref.bounds(indptr, norm)
    for entry in (0, expected[0].size // 2, expected[0].size - 1):
        for sign in (1, -1):
            off = expected[4].copy()
            off[entry] *= 1 + sign * 1.5 * b[entry]
            with pytest.raises(AssertionError, match="no state"):
                ss.match_state(off, expected, indptr, norm)
    for bad in (np.nan, np.inf, 0.0):
        off = _as_device(expected[4]).copy()
        off[3] = bad
        with pytest.raises(AssertionError, match="no state"):
            ss.match_state(off, expected, indptr, norm)
    with pytest.raises(AssertionError, match="entries"):
        ss.match_state(_as_device(expected[4])[:-1], expected, indptr, norm)


def test_idf_vectors_are_recognised_and_held_to_their_bound(corpus):
    for smooth in (True, False):
        vectors = corpus.idf_vectors(smooth)
        assert ss.assert_vectors_separable(vectors) >= 64
        for j, v in enumerate(vectors):
            assert ss.match_vector(_as_device(v), vectors) == j
        off = vectors[2].copy()
        off[5] += 2.5 * 2.0 ** -24 * np.abs(vectors[2]).max()
        with pytest.raises(AssertionError, match="no state"):
            ss.match_vector(off, vectors)
        if not smooth:                                              # a column nobody holds has weight 0, not a small number
            assert (vectors[0] == 0).any()
            off = _as_device(vectors[0]).copy()
            off[np.flatnonzero(vectors[0] == 0)[0]] = 1e-30
            with pytest.raises(AssertionError, match="no state"):
                ss.match_vector(off, vectors)


def test_a_sequence_that_goes_backwards_is_refused():
    assert ss.check_order([0, 0, 1, 1, 4, 6, 6]) == [0, 0, 1, 1, 4, 6, 6]
    assert ss.check_order([]) == [] and ss.check_order([3]) == [3]
    for seq in ([0, 1, 0], [2, 3, 3, 2], [6, 5], [0, 4, 3, 6]):
        with pytest.raises(AssertionError, match="after call"):
            ss.check_order(seq)
    assert ss.check_window(2, 2, 3) == 2 and ss.check_window(3, 2, 3) == 3
    for state, lo, hi in ((1, 2, 3), (4, 2, 3)):                   # a stale state; a state from the future
        with pytest.raises(AssertionError, match="updates had returned"):
            ss.check_window(state, lo, hi)


class _GrowingCounter:
    """latok_counter_read of a counter that another thread keeps updating: after each of the first ``grow`` calls one more word is held.
    The capacity protocol is the header's: too small -> nothing but the two totals is written, LATOK_ERR_INVALID."""

    def __init__(self, words, grow):
        self.words, self.held, self.grow, self.calls = words, len(words) - grow, grow, []

    def latok_counter_read(self, handle, words_out, bytes_cap, word_off_out, counts_out, cap, n_words_out, n_bytes_out):
        import ctypes as C
        held = self.words[:self.held]
        if len(self.calls) < self.grow:
            self.held += 1
        self.calls.append((cap, bytes_cap))
        n_words_out._obj.value, n_bytes_out._obj.value = len(held), sum(map(len, held))
        if len(held) > cap or sum(map(len, held)) > bytes_cap:
            return -1
        raw = b"".join(held)
        C.memmove(words_out.value, raw, len(raw))
        off = np.zeros(len(held) + 1, np.int64)
        off[1:] = np.cumsum([len(w) for w in held])
        C.memmove(word_off_out.value, off.ctypes.data, off.nbytes)
        counts = np.arange(1, len(held) + 1, dtype=np.uint64)
        if len(held):
            C.memmove(counts_out.value, counts.ctypes.data, counts.nbytes)
        return 0


@pytest.mark.parametrize("grow", [0, 1, 3])
def test_counter_items_follows_a_counter_that_grows_between_size_query_and_read(grow):
    """TokenCounter.items() is two library calls; on a counter that contexts share, an update of another thread may land between them.
    The read then reports the larger need (and writes nothing): items() reads again with it and returns one state of the counter."""
    from latok_amd import batch
    words = [b"alpha", b"be", b"gamma", b"d", b"epsilon", b"zeta"]
    fake = _GrowingCounter(words, grow)
    tc = object.__new__(batch.TokenCounter)
    tc._lib, tc.handle = fake, 1
    try:
        got, counts = tc.items()
    finally:
        tc.handle = None                                            # (nothing to destroy)
    assert got == words and counts.tolist() == list(range(1, len(words) + 1)) and counts.dtype == np.uint64     # what the last read saw
    assert fake.calls[0] == (0, 0) and len(fake.calls) == 2 + grow
    assert all(b[0] > a[0] for a, b in zip(fake.calls[1:], fake.calls[2:]))      # every repeat asked with the larger need


class _CountingLib:
    """a library that has nothing but one destroy call: it counts, and fails when told to"""

    def __init__(self, destroy, fail=False):
        self.destroyed, self.fail = [], fail
        setattr(self, destroy, self._destroy)

    def _destroy(self, handle):
        self.destroyed.append(handle)
        if self.fail:
            raise RuntimeError("destroy failed")
        return 0


# class, its destroy call, the argument name of its handle lookup (None: it has none), the text of _open() after close()
HANDLE_CLASSES = [("Vocab", "latok_vocab_destroy", "vocab", "vocab must be an open latok_amd.batch.Vocab"),
                  ("WordPiece", "latok_wordpiece_destroy", "wp", "wp must be an open latok_amd.batch.WordPiece"),
                  ("Idf", "latok_idf_destroy", "idf", "the idf is closed"),
                  ("TokenCounter", "latok_counter_destroy", None, "the TokenCounter is closed")]
LOOKUP_TEXTS = {"vocab": "vocab must be an open latok_amd.batch.Vocab", "wp": "wp must be an open latok_amd.batch.WordPiece",
                "idf": "idf must be an open latok_amd.batch.Idf or None"}


def _fake(name, destroy, fail=False):
    from latok_amd import batch
    cls = getattr(batch, name)
    obj = cls.__new__(cls)
    obj._lib, obj.handle = _CountingLib(destroy, fail), 41
    return obj, obj._lib


@pytest.mark.parametrize("name,destroy,arg,closed_text", HANDLE_CLASSES)
def test_the_four_handle_classes_share_one_lifecycle(name, destroy, arg, closed_text):
    import re
    from latok_amd import batch
    cls = getattr(batch, name)
    obj, lib = _fake(name, destroy)
    assert obj._open() == 41
    if arg:
        assert batch._handle_of(cls, obj, arg, arg == "idf") == 41
    obj.close()
    assert obj.handle is None and lib.destroyed == [41]
    obj.close()
    assert lib.destroyed == [41]                                    # close() twice destroys once
    obj.__del__()
    assert lib.destroyed == [41]                                    # ... and __del__ after close() destroys nothing
    with pytest.raises(ValueError, match="^%s$" % re.escape(closed_text)):
        obj._open()
    if arg:
        for bad in (obj, object(), 41) + (() if arg == "idf" else (None,)):
            with pytest.raises(ValueError, match="^%s$" % re.escape(LOOKUP_TEXTS[arg])):
                batch._handle_of(cls, bad, arg, arg == "idf")

    obj, lib = _fake(name, destroy)
    with obj as entered:
        assert entered is obj and lib.destroyed == []
    assert lib.destroyed == [41] and obj.handle is None             # leaving the block destroys once
    assert obj.__exit__(None, None, None) is False and lib.destroyed == [41]

    obj, lib = _fake(name, destroy, fail=True)
    obj.__del__()                                                   # swallows what destroy raises
    assert lib.destroyed == [41] and obj.handle is None
    obj, lib = _fake(name, destroy, fail=True)
    with pytest.raises(RuntimeError, match="destroy failed"):
        obj.close()                                                 # ... close() itself does not; the handle is gone all the same
    assert obj.handle is None

    bare = cls.__new__(cls)                                         # what the host tests build: nothing but a handle
    bare.handle = None
    bare.close()
    bare.__del__()
    with pytest.raises(ValueError, match="^%s$" % re.escape(closed_text)):
        bare._open()


def test_the_idf_lookup_takes_none():
    from latok_amd import batch
    assert batch._handle_of(batch.Idf, None, "idf", True) is None


def _same_array(got, want, dtype):
    assert isinstance(got, np.ndarray) and got.dtype == dtype and got.flags.c_contiguous and got.tolist() == want, (got, want)


def test_the_word_packer_yields_the_arrays_the_create_calls_take():
    from latok_amd import batch
    data, off, ids = batch._pack_words([], None)
    _same_array(data, [], np.uint8), _same_array(off, [0], np.int64)
    assert ids is None
    data, off, ids = batch._pack_words([], [])                      # (no word: an empty float array is no wrong dtype)
    _same_array(ids, [], np.int32)
    data, off, ids = batch._pack_words([b""], [7])
    _same_array(data, [], np.uint8), _same_array(off, [0, 0], np.int64), _same_array(ids, [7], np.int32)
    # str goes through UTF-8 with surrogatepass, bytes stay as they are (valid or not)
    data, off, ids = batch._pack_words(["a\ud800", b"\xffz", bytearray(b""), "é"], np.array([5, -1, -2 ** 31, 2 ** 31 - 1], np.int64))
    _same_array(data, [0x61, 0xED, 0xA0, 0x80, 0xFF, 0x7A, 0xC3, 0xA9], np.uint8)
    _same_array(off, [0, 4, 6, 6, 8], np.int64)
    _same_array(ids, [5, -1, -2 ** 31, 2 ** 31 - 1], np.int32)
    _same_array(batch._pack_words(iter([b"x", b"y"]), np.arange(4, dtype=np.uint16)[::2])[2], [0, 2], np.int32)    # a generator; strided ids
    for bad in ([1], [1, 2, 3], [[1, 2]], [1.0, 2.0], ["1", "2"], [None, 1]):
        with pytest.raises(ValueError, match="^ids must be one integer per word$"):
            batch._pack_words([b"x", b"y"], bad)
    for bad in ([0, 2 ** 31], [-2 ** 31 - 1, 0], np.array([0, 2 ** 31], np.uint32)):
        with pytest.raises(ValueError, match="^ids must fit int32$"):
            batch._pack_words([b"x", b"y"], bad)
    # Idf.load shares the range check, with its own words
    _same_array(batch._int32_each(np.array([3, 0], np.int64), 2, "df", "column"), [3, 0], np.int32)
    with pytest.raises(ValueError, match="^df must be one integer per column$"):
        batch._int32_each([1.0, 2.0], 2, "df", "column")
    with pytest.raises(ValueError, match="^df must fit int32$"):
        batch._int32_each([0, 2 ** 31], 2, "df", "column")


def test_a_corpus_that_cannot_tell_its_states_apart_fires_the_precondition(corpus):
    # a single-entry row under L2 is 1.0 in every state
    indptr, indices, data = ss.rows_csr([[0, 0, 5, 12], [7]])
    vectors = corpus.idf_vectors(True)
    expected = [ref.weigh(indptr, indices, data, v, False, "l2") for v in vectors]
    with pytest.raises(AssertionError, match="cannot tell them apart"):
        ss.assert_separable(expected, indptr, "l2")
    assert ss.assert_separable([ref.weigh(indptr, indices, data, v, False, None) for v in vectors], indptr, None) >= 64
    # columns of one df: the L2 row does not move with n_docs
    indptr, indices, data = ss.rows_csr([[6, 6, 7]])
    assert corpus.df[0][6] == corpus.df[0][7]
    with pytest.raises(AssertionError, match="cannot tell them apart"):
        ss.assert_separable([ref.weigh(indptr, indices, data, v, False, "l2") for v in vectors], indptr, "l2")
    # an empty row separates nothing
    indptr, indices, data = ss.rows_csr([[0, 5, 12], []])
    with pytest.raises(AssertionError, match="cannot tell them apart"):
        ss.assert_separable([ref.weigh(indptr, indices, data, v, False, None) for v in vectors], indptr, None)
    # two updates that barely move n_docs: closer than 64 bounds
    close = [ref.idf(corpus.df[0], n, True) for n in (10 ** 7, 10 ** 7 + 1)]
    indptr, indices, data = corpus.csr
    with pytest.raises(AssertionError, match="cannot tell them apart"):
        ss.assert_separable([ref.weigh(indptr, indices, data, v, False, None) for v in close], indptr, None)
    with pytest.raises(AssertionError, match="bounds"):
        ss.assert_vectors_separable(close)
    # and the matcher itself refuses to pick between states it cannot tell apart
    same = [corpus.expected(True, None)[0]] * 2
    with pytest.raises(AssertionError, match="states \\[0, 1\\]"):
        ss.match_state(same[0], same, indptr, None)
