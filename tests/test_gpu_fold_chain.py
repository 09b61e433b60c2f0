"""Folding chained in front of the byte-space token calls (latok_amd.batch: the ``fold=`` keyword of the WordPiece, token-id and
term-count calls): the batch is folded on the device and the folded bytes, left there, are the next call's input.  Each chained call
must equal the same call with ``fold=0`` on blobs folded by tests/helpers/fold_ref.py -- ids, indptr and spans, the spans being byte
ranges of the FOLDED string.  Where the `tokenizers` package is installed, the chained padded call is held to BertWordPieceTokenizer
on lines whose words latok and BERT's pre-tokenizer cut alike."""
import random

import numpy as np
import pytest

from helpers import fold_ref as ref

pytestmark = pytest.mark.gpu

WORDS = ["Café", "RÉSUMÉ", "naïve", "Ångström", "Übergröße", "Tiếng", "Việt", "Ελληνικά", "Άλφα", "Привет", "МОСКВА", "한국어", "서울", "İstanbul",
         "plain", "MiXeD", "unaffable", "Unaffable", "UNAFFABLE", "ünaffable", "日本語", "x", "A"]
FOLDS = (ref.UNCASED, ref.LOWER, ref.ALL)


def _lines(seed, n=300):
    rng = random.Random(seed)
    return [" ".join(rng.choice(WORDS) for _ in range(rng.randint(0, 12))).encode() for _ in range(n)] + [b"", b"  ", "À".encode() * 3000]


def _vocab_words(fold):
    """folded words, their pieces and a few that never match"""
    words = ["[UNK]", "[CLS]", "[SEP]", "[PAD]"]
    for w in WORDS:
        f = ref.fold_bytes(w.encode(), fold).decode().strip()
        for part in f.split():
            words += [part, part[:2], "##" + part[2:]] if len(part) > 3 else [part]
    return [w for i, w in enumerate(words) if w and w != "##" and w not in words[:i]]


@pytest.mark.parametrize("fold", FOLDS)
def test_wordpiece_calls_equal_the_calls_on_folded_blobs(gpu, fold):
    from latok_amd import batch
    blobs = _lines(fold)
    folded = ref.fold_blobs(blobs, fold)
    with batch.WordPiece(_vocab_words(fold)) as wp:
        got = batch.wordpiece_ids_utf8_batch(blobs, wp, unk_id=0, fold=fold)
        want = batch.wordpiece_ids_utf8_batch(folded, wp, unk_id=0)
        for g, w, what in zip(got, want, ("indptr", "ids", "spans")):
            assert g.dtype == w.dtype and np.array_equal(g, w), what
        assert (got[1] != 0).mean() > 0.5                                        # the vocabulary is hit: the comparison is not of unks
        plain = batch.wordpiece_ids_utf8_batch(blobs, wp, unk_id=0)
        assert not np.array_equal(plain[1], got[1])                              # ... and folding matters
        texts = [b.decode() for b in blobs]
        for g, w in zip(batch.wordpiece_ids_batch(texts, wp, unk_id=0, fold=fold), want):
            assert np.array_equal(g, w)
        for kw in (dict(max_length=16, cls_id=1, sep_id=2, pad_id=3, unk_id=0), dict(max_length=5, unk_id=0)):
            g_ids, g_mask = batch.wordpiece_encode_utf8_batch(blobs, wp, fold=fold, **kw)
            w_ids, w_mask = batch.wordpiece_encode_utf8_batch(folded, wp, **kw)
            assert np.array_equal(g_ids, w_ids) and np.array_equal(g_mask, w_mask)
        assert batch.wordpiece_encode_utf8_batch([], wp, max_length=4, fold=fold)[0].shape == (0, 4)


@pytest.mark.parametrize("fold", FOLDS)
def test_vocabulary_calls_equal_the_calls_on_folded_blobs(gpu, fold):
    from latok_amd import batch
    blobs = _lines(100 + fold)
    folded = ref.fold_blobs(blobs, fold)
    words = sorted({p for w in WORDS for p in ref.fold_bytes(w.encode(), fold).split()})[::2]
    with batch.Vocab(words) as vocab:
        got, want = batch.token_ids_utf8_batch(blobs, vocab, fold=fold), batch.token_ids_utf8_batch(folded, vocab)
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
        assert sum(int((g >= 0).sum()) for g in got) > 100
        got, want = batch.term_counts_utf8_batch(blobs, vocab, fold=fold), batch.term_counts_utf8_batch(folded, vocab)
        for g, w, what in zip(got, want, ("indptr", "indices", "data", "oov")):
            assert g.dtype == w.dtype and np.array_equal(g, w), what
        assert batch.token_ids_utf8_batch([], vocab, fold=fold) == []
    got = batch.hashed_term_counts_utf8_batch(blobs, n_features=1 << 12, seed=3, fold=fold)
    want = batch.hashed_term_counts_utf8_batch(folded, n_features=1 << 12, seed=3)
    for g, w, what in zip(got, want, ("indptr", "indices", "data")):
        assert g.dtype == w.dtype and np.array_equal(g, w), what


def test_the_uncased_vocabulary_of_the_readme(gpu):
    from latok_amd import batch
    with batch.WordPiece(["[UNK]", "un", "##aff", "##able", "a"], prefix=b"##", max_chars=100) as wp:
        _, want, _ = batch.wordpiece_ids_utf8_batch([b"unaffable"], wp, unk_id=0)
        assert want.tolist() == [1, 2, 3]
        blobs = [t.encode() for t in ("Unaffable", "UNAFFABLE", "ünaffable")]
        indptr, ids, spans = batch.wordpiece_ids_utf8_batch(blobs, wp, unk_id=0, fold=batch.FOLD_UNCASED)
        assert indptr.tolist() == [0, 3, 6, 9] and ids.tolist() == [1, 2, 3] * 3
        assert spans.tolist() == [[0, 2], [2, 5], [5, 9]] * 3                    # byte ranges of the FOLDED string: ü is one byte there
        indptr, ids, _ = batch.wordpiece_ids_utf8_batch(blobs, wp, unk_id=0)
        assert indptr.tolist() == [0, 1, 2, 3] and ids.tolist() == [0, 0, 0]


def test_chained_padded_call_equals_bert_wordpiece_tokenizer(gpu, tmp_path):
    tk = pytest.importorskip("tokenizers")
    from latok_amd import batch
    fold = batch.FOLD_UNCASED
    words = [w for w in _vocab_words(fold) if not any(0x4E00 <= ord(c) <= 0x9FFF for c in w)]
    path = tmp_path / "vocab.txt"
    path.write_text("".join(w + "\n" for w in words), encoding="utf-8")
    bert = tk.BertWordPieceTokenizer(str(path), lowercase=True, strip_accents=True, clean_text=False, handle_chinese_chars=False)
    rng = random.Random(9)
    plain = [w for w in WORDS if w != "日本語"]
    lines = [" ".join(rng.choice(plain) for _ in range(rng.randint(1, 9))) for _ in range(200)]
    cls_id, sep_id, unk_id = words.index("[CLS]"), words.index("[SEP]"), words.index("[UNK]")
    with batch.WordPiece.from_vocab_file(str(path)) as wp:
        ids, mask = batch.wordpiece_encode_utf8_batch([t.encode() for t in lines], wp, max_length=64, cls_id=cls_id, sep_id=sep_id,
                                                      pad_id=words.index("[PAD]"), unk_id=unk_id, fold=fold)
    for row, m, line in zip(ids, mask, lines):
        assert row[:int(m.sum())].tolist() == bert.encode(line).ids, line
