"""The two routes of the sized byte-space calls of latok_amd.batch agree bit for bit: a call with ``fold=F`` (the batch folded into
device memory, the call on device buffers) returns what the same call with ``fold=0`` returns on ``fold_utf8_batch(blobs, F)`` (host
arrays in, host arrays out) -- values, dtypes and shapes.  Both routes are written once against one batch interface; this pins that
they stay one.  The families: token ids, term counts and TF-IDF (vocabulary and hashed, words and word bigrams), Idf.update_utf8,
WordPiece ids and the padded WordPiece block."""
import numpy as np
import pytest

from helpers import fold_ref as ref

F = ref.LOWER | ref.STRIP_MARKS
# folding changes the byte length in both directions: É (2 bytes) -> e (1), Ⱥ (2 bytes) -> ⱥ (3)
SHRINKS, GROWS, BOTH = "CAFÉ É Éa".encode(), "Ⱥ Ⱥb xȺ".encode(), "Éa Ⱥb É Ⱥ".encode()
WORDS = ["Café", "Ⱥb", "RÉSUMÉ", "x", "naïve", "É", "plain", "Ⱥ", "Ångström", "a"]


def _crossing():
    """strings of mixed text, 4097 + 3 bytes in all: the batch crosses a tile boundary"""
    blobs, total, i = [], 0, 0
    while total < 4000:
        blobs.append(" ".join(WORDS[(i + 3 * k) % len(WORDS)] for k in range(1 + i % 9)).encode())
        total += len(blobs[-1])
        i += 1
    return blobs + ["Ⱥb É ".encode() + b"Q" * (4100 - total - 7)]


BATCHES = {"none": [], "one_empty": [b""], "blank": [b"", b"  ", b"x"], "lengths": [SHRINKS, GROWS, BOTH], "crossing": _crossing()}
VOCAB = ["cafe", "e", "ea", "x", "resume", "naive", "plain", "ⱥ", "ⱥb", "xⱥ", "a", "e ea", "ⱥ ⱥb", "cafe e", "x naive"]
PIECES = ["[UNK]", "[CLS]", "[SEP]", "[PAD]", "ca", "##fe", "e", "##a", "x", "##ⱥ", "re", "##sume", "na", "##ive", "plain", "ⱥ", "##b", "a"]


def test_the_chosen_strings_change_length_under_the_fold():
    assert len(ref.fold_bytes(SHRINKS, F)) < len(SHRINKS) and len(ref.fold_bytes(GROWS, F)) > len(GROWS)
    both = ref.fold_bytes(BOTH, F)
    assert both == "ea ⱥb e ⱥ".encode() and len(both) == len(BOTH)            # one letter shrinks, one grows, twice each
    total = sum(len(b) for b in BATCHES["crossing"])
    assert total == 4100 and sum(len(b) for b in ref.fold_blobs(BATCHES["crossing"], F)) != total
    for w in VOCAB + [p.lstrip("#") for p in PIECES[4:]]:
        assert ref.fold_bytes(w.encode(), F) == w.encode(), w                   # the vocabularies are folded already


def _same(got, want, what):
    if isinstance(want, (tuple, list)):
        assert type(got) is type(want) and len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, "%s[%d]" % (what, i))
    else:
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), what


@pytest.fixture(scope="module")
def objects(gpu):
    from latok_amd import batch
    with batch.Vocab(VOCAB) as vocab, batch.WordPiece(PIECES) as wp:
        yield batch, vocab, wp


@pytest.fixture(scope="module", params=sorted(BATCHES))
def routes(request, objects):
    """(batch, vocab, wp, check, n_str): check(what, f) holds f(blobs, F) to f(the blobs folded by fold_utf8_batch, 0)"""
    batch, vocab, wp = objects
    blobs = BATCHES[request.param]
    folded = batch.fold_utf8_batch(blobs, F)
    assert folded == ref.fold_blobs(blobs, F)

    def check(what, f):
        got, want = f(blobs, F), f(folded, 0)
        _same(got, want, "%s on %s" % (what, request.param))
        return got

    return batch, vocab, wp, check, len(blobs)


@pytest.mark.gpu
def test_token_ids(routes):
    batch, vocab, _, check, _ = routes
    got = check("token ids", lambda b, fold: batch.token_ids_utf8_batch(b, vocab, unk_id=-3, fold=fold))
    assert all(a.dtype == np.int32 for a in got)


@pytest.mark.gpu
@pytest.mark.parametrize("ngram_range", [(1, 1), (1, 2)])
def test_term_counts(routes, ngram_range):
    batch, vocab, _, check, _ = routes
    got = check("term counts", lambda b, fold: batch.term_counts_utf8_batch(b, vocab, fold=fold, ngram_range=ngram_range))
    assert len(got) == 4 and got[0].dtype == np.int64 and got[1].dtype == np.int32
    got = check("hashed term counts",
                lambda b, fold: batch.hashed_term_counts_utf8_batch(b, n_features=1 << 10, seed=5, fold=fold, ngram_range=ngram_range))
    assert len(got) == 3


@pytest.mark.gpu
def test_idf_update_and_tfidf(routes):
    batch, vocab, _, check, n_str = routes
    for kw, n_cols in ((dict(vocab=vocab), len(VOCAB)), (dict(n_features=1 << 10, seed=5), 1 << 10)):
        with batch.Idf(n_cols) as via_fold, batch.Idf(n_cols) as via_host:
            idfs = {F: via_fold, 0: via_host}
            for ngram_range in ((1, 1), (1, 2)):
                check("Idf.update_utf8", lambda b, fold: np.array(idfs[fold].update_utf8(b, fold=fold, ngram_range=ngram_range, **kw)))
            assert via_fold.n_docs == via_host.n_docs == 2 * n_str
            assert np.array_equal(via_fold.df(), via_host.df())
            for ngram_range in ((1, 1), (1, 2)):
                if "vocab" in kw:
                    got = check("tfidf", lambda b, fold: batch.tfidf_utf8_batch(b, vocab, via_host, fold=fold, ngram_range=ngram_range))
                    assert len(got) == 4 and got[2].dtype == np.float32
                else:
                    got = check("hashed tfidf", lambda b, fold: batch.hashed_tfidf_utf8_batch(b, idf=via_host, fold=fold, ngram_range=ngram_range, **kw))
                    assert len(got) == 3 and got[2].dtype == np.float32


@pytest.mark.gpu
def test_wordpiece(routes):
    batch, _, wp, check, _ = routes
    got = check("WordPiece ids", lambda b, fold: batch.wordpiece_ids_utf8_batch(b, wp, unk_id=0, fold=fold))
    assert len(got) == 3 and got[2].shape == (got[1].size, 2)
    for kw in (dict(max_length=7, cls_id=1, sep_id=2, pad_id=3), dict(max_length=4)):
        ids, mask = check("WordPiece encode", lambda b, fold: batch.wordpiece_encode_utf8_batch(b, wp, unk_id=0, fold=fold, **kw))
        assert ids.shape == mask.shape and ids.shape[1] == kw["max_length"]
