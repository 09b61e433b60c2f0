#!/usr/bin/env python3
"""Writes the recorded cases of GPT-2's pre-tokenizer under tests/golden/.  Run once by hand where the ``regex`` and ``tokenizers``
packages are installed; no test runs it.

    python tools/make_pretok_golden.py

  pretok_worked.json       a worked table: strings with the BYTE offsets at which ``regex.finditer`` with GPT-2's pattern starts a match
  pretok_gpt2/vocab.json   a byte-level BPE of a few hundred merges, trained by ``tokenizers`` (ByteLevel pre-tokenizer, GPT-2's regex) on a
  pretok_gpt2/merges.txt   synthetic corpus, saved in GPT-2's two files, with one special token
  pretok_gpt2_cases.json   texts with the ``ids`` and the ``offsets`` (in CHARACTERS, as the package reports them) that tokenizer gives

Before anything is written the tool asserts that tests/helpers/pretok_ref.py gives the worked table's starts and that pretok_ref +
bpe_ref.cut over ``BPE.gpt2_word_list`` of the two files reproduce every id and every offset of every text; no text may be left out."""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PATTERN = r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"
FIXED = ["", " ", "  ", "\n", " \n ", "\t\t", "　", "　 　", "don't", "I'll we've you're she'd I'm it's", "DON'T 'S", "it' s", "'tis", " 'll", "a 's",
         "a\n's", "a　's", "x''s", "1's 2'd", "hello  world", "hello   world ", "a\n\nb", "a \n b", "tab\there", "日本語のテキスト、です。", "日本 語", "中文 123 abc",
         "🤓 ok 🤓🤓", "price: $12.50!", "http://a.b/c?d=e&f", "me@x.org", "x²+y³", "٣٤ digits", "①②③", "über naïve café", "end. ", "end.  ", " lead",
         "  lead", "\nlead", "a b", "a  b", "a b", "a…b", "'", "''", "'s", "s'", "'s's", "a'ss", "a'rex", "a'r", "a'l", "a'lll",
         "\x1c\x1d", "a\x85b", "C++ & C#", "snake_case_name", "e=mc^2", "1,000,000.00", "A.B.C.", "what?! no...", "(paren) [brack] {brace}"]
WORDS = ["the", "of", "and", "to", "in", "is", "that", "for", "it", "was", "with", "token", "tokens", "model", "models", "byte", "bytes", "pair",
         "merge", "merges", "rank", "space", "spaces", "number", "numbers", "device", "kernel", "string", "strings", "don", "can", "won", "they",
         "we", "you", "I", "she", "he", "hello", "world", "Hello", "World", "über", "café", "naïve", "日本", "語", "中文", "テキスト"]
SEPS = [" ", " ", " ", " ", "  ", "\n", ", ", ". ", "! ", "? ", "\t", " - ", "　", "'s ", "'t ", "'re ", "'ll ", "'ve ", "'m ", "'d ", ": ", "; "]
EXTRA = ["123", "2024", "3.14", "🤓", "http://u.rl/x", "a@b.c", "$5", "#tag", "(x)", "100%"]


def synthetic(rng, n_words):
    out = []
    for _ in range(n_words):
        out.append(rng.choice(EXTRA) if rng.random() < 0.12 else rng.choice(WORDS))
        out.append(rng.choice(SEPS))
    if rng.random() < 0.5:
        out.pop()
    return "".join(out)


def main():
    import regex
    import tokenizers
    from tokenizers import Tokenizer, models, pre_tokenizers, trainers
    from helpers import bpe_ref, pretok_ref
    from latok_amd import batch

    gold = os.path.join(ROOT, "tests", "golden")
    rng = random.Random(21)
    pat = regex.compile(PATTERN)
    # (a) the worked table
    table = []
    for text in FIXED + [pretok_ref.random_text(rng, 30) for _ in range(140)]:
        starts = [len(text[:m.start()].encode()) for m in pat.finditer(text)]
        assert pretok_ref.starts(text.encode()) == starts, text
        table.append({"text": text, "starts": starts})
    # (b) the vocabulary
    corpus = [synthetic(rng, rng.randint(3, 30)) for _ in range(3000)]
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
    trainer = trainers.BpeTrainer(vocab_size=256 + 1 + 400, special_tokens=["<|endoftext|>"], initial_alphabet=pre_tokenizers.ByteLevel.alphabet(),
                                  show_progress=False)
    tok.train_from_iterator(corpus, trainer)
    model_dir = os.path.join(gold, "pretok_gpt2")
    os.makedirs(model_dir, exist_ok=True)
    tok.model.save(model_dir)
    words, ids, specials = batch.BPE.gpt2_word_list(os.path.join(model_dir, "vocab.json"), os.path.join(model_dir, "merges.txt"))
    assert specials == {"<|endoftext|>": tok.token_to_id("<|endoftext|>")} and len(words) == len(set(words)) > 400, (specials, len(words))
    d = bpe_ref.rank_dict(words)
    # (c) the texts
    texts = FIXED + [synthetic(rng, rng.randint(1, 12)) for _ in range(110)] + [pretok_ref.random_text(rng, 30) for _ in range(60)]
    cases = []
    for text in texts:
        enc = tok.encode(text, add_special_tokens=False)
        blob = text.encode()
        char_of = []                       # the character that holds each byte
        for i, ch in enumerate(text):
            char_of += [i] * len(ch.encode())
        got_ids, got_off = [], []
        for a, e in pretok_ref.pretokens(blob):
            for pid, p0, p1 in bpe_ref.cut(blob[a:e], d, 4096, -1, ids):
                got_ids.append(pid)
                got_off.append([char_of[a + p0], char_of[a + p1 - 1] + 1])
        assert got_ids == list(enc.ids), (text, got_ids, enc.ids)
        assert got_off == [list(o) for o in enc.offsets], (text, got_off, enc.offsets)
        cases.append({"text": text, "ids": list(enc.ids), "offsets": [list(o) for o in enc.offsets]})
    for name, doc in (("pretok_worked.json", {"pattern": PATTERN, "library": "regex " + regex.__version__, "cases": table}),
                      ("pretok_gpt2_cases.json", {"library": "tokenizers " + tokenizers.__version__,
                                                  "model": "models.BPE trained with pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)",
                                                  "offsets": "characters, as the package reports them: a piece covers every character it holds a byte of",
                                                  "cases": cases})):
        path = os.path.join(gold, name)
        with open(path, "w", encoding="utf-8") as f:
            json.dump(doc, f, ensure_ascii=False, separators=(",", ":"))
            f.write("\n")
        print("%s: %d cases, %d bytes" % (path, len(doc["cases"]), os.path.getsize(path)))
    print("%s: %d words, %d pieces over %d texts" % (model_dir, len(words), sum(len(c["ids"]) for c in cases), len(cases)))


if __name__ == "__main__":
    main()
