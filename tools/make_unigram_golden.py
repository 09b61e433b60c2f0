#!/usr/bin/env python3
"""Writes tests/golden/unigram_hf_cases.json: what ``tokenizers.models.Unigram`` (the Hugging Face implementation of SentencePiece's
Unigram search), with no normalizer and no pre-tokenizer, gives for single words over small vocabularies -- ids and BYTE offsets.  Run
once by hand where the ``tokenizers`` package is installed; no test runs it.

    python tools/make_unigram_golden.py [out.json]

Every vocabulary has ``<unk>`` (score 0) at position 0, which no word can spell, so that ids are positions in the recorded list.
Scores are multiples of 1/8: the package adds in float64 where the library adds in float32, and such sums are exact in both.  Every
word is drawn from ONE script class (lower-case Latin with é, or CJK) and is asserted to be exactly one token of the project's CPU
tokenizer.  A word is recorded twice: as it is, and from the input "▁" + word (offsets then count the marker's 3 bytes)."""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

MARKER = "▁"
LATIN, LATIN_UNKNOWN = "abcé", "z"
CJK, CJK_UNKNOWN = "日本語中", "字"


def byte_offsets(text, offsets):
    at = [0]
    for ch in text:
        at.append(at[-1] + len(ch.encode()))
    return [[at[s], at[e]] for s, e in offsets]


def main():
    import tokenizers
    from tokenizers import Tokenizer
    from tokenizers.models import Unigram
    import latok_oracle as dt   # the CPU restatement of the tokenizer (make -C oracle restate)

    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "unigram_hf_cases.json")
    rng = random.Random(20)
    vocabularies = []
    # (alphabet, unknown letter, words, every single character is a word, words that begin with the marker)
    plans = [(LATIN, LATIN_UNKNOWN, 6, True, 0), (LATIN, LATIN_UNKNOWN, 10, True, 4), (LATIN, LATIN_UNKNOWN, 14, False, 5),
             (LATIN, LATIN_UNKNOWN, 3, False, 0), (LATIN, LATIN_UNKNOWN, 12, True, 6), (LATIN, LATIN_UNKNOWN, 8, False, 8),
             (CJK, CJK_UNKNOWN, 8, True, 3), (CJK, CJK_UNKNOWN, 10, False, 4), (CJK, CJK_UNKNOWN, 5, True, 0), (LATIN, LATIN_UNKNOWN, 1, False, 1)]
    for alphabet, unknown, n_words, singles, n_marked in plans:
        words = list(alphabet) if singles else []
        while len(words) < (len(alphabet) if singles else 0) + n_words:
            w = "".join(rng.choice(alphabet) for _ in range(rng.choice((1, 2, 2, 3, 3, 4))))
            if w not in words:
                words.append(w)
        marked = [MARKER + w for w in rng.sample(words, min(n_marked, len(words)))]
        if n_marked and rng.random() < 0.6:
            marked.append(MARKER)
        words += marked
        rng.shuffle(words)
        vocab = [("<unk>", 0.0)] + [(w, -rng.randint(1, 64) / 8.0) for w in words]
        tok = Tokenizer(Unigram(vocab, unk_id=0, byte_fallback=False))
        cases = []
        letters = alphabet + unknown
        for _ in range(30):
            word = "".join(rng.choice(letters if rng.random() < 0.4 else alphabet) for _ in range(rng.randint(1, 9)))
            assert list(dt.tokenize(word)) == [word], word
            for text in (word, MARKER + word):
                enc = tok.encode(text, add_special_tokens=False)
                cases.append({"word": word, "marked": text != word, "ids": list(enc.ids), "offsets": byte_offsets(text, enc.offsets)})
        vocabularies.append({"words": [w for w, _ in vocab], "scores": [s for _, s in vocab], "unk_id": 0, "cases": cases})
    doc = {"library": "tokenizers", "version": tokenizers.__version__, "model": "tokenizers.models.Unigram, no normalizer, no pre-tokenizer",
           "marker": MARKER, "unk_score": "min(scores) - 10", "fuse_unk": True, "vocabularies": vocabularies}
    with open(out_path, "w", encoding="utf-8") as f:
        json.dump(doc, f, ensure_ascii=False, indent=None, separators=(",", ":"))
        f.write("\n")
    print("%s: %d vocabularies, %d cases, %d bytes" % (out_path, len(vocabularies), sum(len(v["cases"]) for v in vocabularies), os.path.getsize(out_path)))


if __name__ == "__main__":
    main()
