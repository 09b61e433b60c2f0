"""The sized byte-space wrappers of latok_amd.batch refuse a bad argument with ValueError before they ask for a device, on the host
route (``fold=0``) and on the folded one alike: ``_lib.ensure_init`` is replaced by a function that raises, and the vocabulary
objects are bare (a handle, no library), so a wrapper that reached the device first would raise something else."""
import pytest

from latok_amd import _lib, batch

FOLDS = (0, batch.FOLD_LOWER | batch.FOLD_STRIP_MARKS)
BLOBS = [b"a b", b""]
BAD_NGRAMS = [dict(ngram_range=(0, 1)), dict(ngram_range=(2, 1)), dict(ngram_range=(1, batch.NGRAM_MAX + 1)), dict(ngram_range=(1, 2.0)),
              dict(ngram_range=(1,)), dict(ngram_range=2), dict(sep=b""), dict(sep=b"ab"), dict(sep="é"), dict(sep=None)]
BAD_FEATURES = [dict(n_features=0), dict(n_features=1 << 31), dict(n_features=2.0), dict(n_features=True)]
BAD_NORM = [dict(norm="l3"), dict(norm=2)]
BAD_UNK = [dict(unk_id=1 << 31), dict(unk_id=-(1 << 31) - 1), dict(unk_id=None), dict(unk_id=1.0)]


class DeviceTouched(Exception):
    pass


class _NoLibrary:
    def __getattr__(self, name):
        raise DeviceTouched(name)


@pytest.fixture
def bare(monkeypatch):
    """(vocab, wp, idf): open objects without a device behind them"""
    def touched(*a, **kw):
        raise DeviceTouched("ensure_init")

    monkeypatch.setattr(_lib, "ensure_init", touched)
    objs = []
    for cls in (batch.Vocab, batch.WordPiece, batch.Idf):
        obj = cls.__new__(cls)
        obj.handle, obj._lib = 1, _NoLibrary()
        objs.append(obj)
    yield objs
    for obj in objs:
        obj.handle = None                                  # (nothing to destroy)


def _csr(blobs):
    return batch.pack_utf8(blobs)


def _wrappers(vocab, wp, idf):
    """name -> (call(fold, **kw), takes fold, the keyword sets it must refuse)"""
    b = batch
    return {
        "token_ids_utf8_batch": (lambda fold, **kw: b.token_ids_utf8_batch(BLOBS, vocab, fold=fold, **kw), True, BAD_UNK),
        "token_ids_utf8_csr": (lambda fold, **kw: b.token_ids_utf8_csr(*_csr(BLOBS), vocab, **kw), False, BAD_UNK),
        "term_counts_utf8_batch": (lambda fold, **kw: b.term_counts_utf8_batch(BLOBS, vocab, fold=fold, **kw), True, BAD_NGRAMS),
        "term_counts_utf8_csr": (lambda fold, **kw: b.term_counts_utf8_csr(*_csr(BLOBS), vocab, **kw), False, BAD_NGRAMS),
        "hashed_term_counts_utf8_batch": (lambda fold, **kw: b.hashed_term_counts_utf8_batch(BLOBS, fold=fold, **kw), True, BAD_NGRAMS + BAD_FEATURES),
        "hashed_term_counts_utf8_csr": (lambda fold, **kw: b.hashed_term_counts_utf8_csr(*_csr(BLOBS), **kw), False, BAD_NGRAMS + BAD_FEATURES),
        "tfidf_utf8_batch": (lambda fold, **kw: b.tfidf_utf8_batch(BLOBS, vocab, idf, fold=fold, **kw), True, BAD_NGRAMS + BAD_NORM),
        "tfidf_utf8_csr": (lambda fold, **kw: b.tfidf_utf8_csr(*_csr(BLOBS), vocab, idf, fold=fold, **kw), True, BAD_NGRAMS + BAD_NORM),
        "hashed_tfidf_utf8_batch": (lambda fold, **kw: b.hashed_tfidf_utf8_batch(BLOBS, idf=idf, fold=fold, **kw), True,
                                    BAD_NGRAMS + BAD_NORM + BAD_FEATURES),
        "hashed_tfidf_utf8_csr": (lambda fold, **kw: b.hashed_tfidf_utf8_csr(*_csr(BLOBS), idf=idf, fold=fold, **kw), True,
                                  BAD_NGRAMS + BAD_NORM + BAD_FEATURES),
        "Idf.update_utf8 (vocab)": (lambda fold, **kw: idf.update_utf8(BLOBS, vocab=vocab, fold=fold, **kw), True,
                                    BAD_NGRAMS + [dict(n_features=8)]),                 # (both of vocab and n_features)
        "Idf.update_utf8 (hashed)": (lambda fold, **kw: idf.update_utf8(BLOBS, **dict(dict(n_features=8), **kw), fold=fold), True,
                                     BAD_NGRAMS + BAD_FEATURES + [dict(n_features=None)]),   # (neither of the two)
        "wordpiece_ids_utf8_batch": (lambda fold, **kw: b.wordpiece_ids_utf8_batch(BLOBS, wp, fold=fold, **kw), True, BAD_UNK),
        "wordpiece_ids_utf8_csr": (lambda fold, **kw: b.wordpiece_ids_utf8_csr(*_csr(BLOBS), wp, **kw), False, BAD_UNK),
        "wordpiece_encode_utf8_batch": (lambda fold, **kw: b.wordpiece_encode_utf8_batch(BLOBS, wp, **dict(dict(max_length=8), **kw), fold=fold), True,
                                        BAD_UNK + [dict(max_length=0), dict(max_length=1 << 31), dict(max_length=8.0), dict(max_length=True),
                                                   dict(max_length=2, cls_id=1, sep_id=2), dict(cls_id=1), dict(sep_id=2), dict(pad_id=None)]),
    }


def test_every_bad_argument_is_a_value_error_before_any_device_call(bare):
    seen = 0
    for name, (call, takes_fold, bad) in _wrappers(*bare).items():
        for fold in FOLDS if takes_fold else (0,):
            for kw in bad:
                with pytest.raises(ValueError):
                    call(fold, **kw)
                    pytest.fail("%s(fold=%d) took %r" % (name, fold, kw))
                seen += 1
            with pytest.raises(DeviceTouched):              # ... and with good arguments the device is what comes next
                call(fold)
    assert seen > 200


def test_the_fold_flags_and_the_objects_are_checked_too(bare):
    vocab, wp, idf = bare
    for name, (call, takes_fold, _) in _wrappers(vocab, wp, idf).items():
        for fold in (-1, 16, 1.0, True, None) if takes_fold else ():
            with pytest.raises(ValueError, match="fold"):
                call(fold)
    closed = batch.Vocab.__new__(batch.Vocab)
    closed.handle = None
    for name in ("token_ids_utf8_batch", "term_counts_utf8_batch", "tfidf_utf8_batch", "Idf.update_utf8 (vocab)"):
        for fold in FOLDS:
            with pytest.raises(ValueError, match="vocab"):
                _wrappers(closed, wp, idf)[name][0](fold)
