#!/usr/bin/env python3
"""Writes the recorded cases of the cl100k / Llama 3 pre-tokenizer under tests/golden/.  Run once by hand where the ``regex`` and
``tokenizers`` packages are installed; no test runs it.

    python tools/make_pretok_cl100k_golden.py

  pretok_cl100k_worked.json            a worked table: strings with the BYTE offsets at which ``regex.finditer`` with the pattern starts a match
  pretok_cl100k/tokenizer.json         a byte-level BPE of a few hundred merges, trained by ``tokenizers`` with the Llama-3-style pre-tokenizer
                                       (Split by the pattern, isolated, then ByteLevel without its regex) on a synthetic corpus, one special token
  pretok_cl100k_cases.json             texts with the ``ids`` and the ``offsets`` (in CHARACTERS, as the package reports them) that tokenizer gives

Before anything is written the tool asserts that tests/helpers/pretok_cl100k_ref.py gives the worked table's starts and that the
reference + bpe_ref.cut over ``BPE.tokenizer_json_word_list`` of the file reproduce every id and every offset of every text; no text may
be left out.  Every character of every text has the same class in tests/golden/pretok_classes.json as in ``regex`` (asserted too: the
two may know different Unicode versions)."""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIXED = ["!\n\n  \n x 1234567  \t!", "", " ", "  ", "\n", "\r\n", " \n ", "\t\t", "　", "　 　", "don't", "I'll we've you're she'd I'm it's", "DON'T 'S 'Re 'lL 'vE",
         "it'ſ long", "'ſ", "a'ſb", "it' s", "'tis", " 'll", "a 's", "a\n's", "a\t's", "a　's", "x''s", "!'s", "1's 2'D", "hello  world", "hello   world ",
         "a\n\nb", "a \n b", "a \r\n\r\n b", "tab\there", "日本語のテキスト、です。", "日本 語", "中文 123 abc", "🤓 ok 🤓🤓", "price: $12.50!", "http://a.b/c?d=e&f",
         "me@x.org", "x²+y³", "٣٤٥٦ digits", "①②③④", "über naïve café", "end. ", "end.  ", " lead", "  lead", "\nlead", "a b", "a  b", "a b", "a…b", "'", "''",
         "'s", "s'", "'s's", "a'ss", "a'rex", "a'r", "a'l", "a'lll", "\x1c\x1d", "a\x85b", "C++ & C#", "snake_case_name", "e=mc^2", "1,000,000.00", "A.B.C.",
         "what?! no...", "(paren) [brack] {brace}", " !", "!!a", "!a", "\ta", " a", "　a", "a!b", "a !b", "1", "12", "123", "1234", "12345", "123456", "1234567",
         "a1234567b", "1 2 3", "１２３４", "1２३٤5", "!\n", "!\n\n\n", "! \n", "!\n \n", "a\n\n", "\n\n", "\n \n", " \n\n ", "  \n  \n  x", "\n  x", "\n  ", "\n  \n",
         "x \t \t y", "x y", "!!\n\r\nx", "'\n", "''\n\n'"]
WORDS = ["the", "of", "and", "to", "in", "is", "that", "for", "it", "was", "with", "token", "tokens", "model", "models", "byte", "bytes", "pair",
         "merge", "merges", "rank", "space", "spaces", "number", "numbers", "device", "kernel", "string", "strings", "don", "can", "won", "they",
         "we", "you", "I", "she", "he", "hello", "world", "Hello", "World", "über", "café", "naïve", "日本", "語", "中文", "テキスト"]
SEPS = [" ", " ", " ", " ", "  ", "\n", "\n\n", ", ", ". ", "! ", "? ", "\t", " - ", "　", "'s ", "'t ", "'RE ", "'ll ", "'Ve ", "'m ", "'d ", ": ", "; ", ".\n", "!\r\n"]
EXTRA = ["123", "2024", "3.14", "1234567", "🤓", "http://u.rl/x", "a@b.c", "$5", "#tag", "(x)", "100%", "65536"]


def synthetic(rng, n_words):
    out = []
    for _ in range(n_words):
        out.append(rng.choice(EXTRA) if rng.random() < 0.15 else rng.choice(WORDS))
        out.append(rng.choice(SEPS))
    if rng.random() < 0.5:
        out.pop()
    return "".join(out)


def main():
    import regex
    import tokenizers
    from tokenizers import Regex, Tokenizer, models, pre_tokenizers, trainers
    from helpers import bpe_ref, pretok_ref
    from helpers import pretok_cl100k_ref as ref
    from latok_amd import batch

    gold = os.path.join(ROOT, "tests", "golden")
    rng = random.Random(22)
    assert ref.PATTERN == batch.BPE.CL100K_PATTERN
    pat = regex.compile(ref.PATTERN)
    classes = {"S": regex.compile(r"\s"), "L": regex.compile(r"\p{L}"), "N": regex.compile(r"\p{N}")}
    seen = set()

    def same_classes(text):
        for ch in set(text) - seen:
            want = "S" if classes["S"].match(ch) else "L" if classes["L"].match(ch) else "N" if classes["N"].match(ch) else "O"
            assert pretok_ref.cp_class(ord(ch)) == want, (hex(ord(ch)), want)
            seen.add(ch)
        return text

    # (a) the worked table
    table = []
    for text in FIXED + [ref.random_text(rng, 30) for _ in range(200)]:
        same_classes(text)
        starts = [len(text[:m.start()].encode()) for m in pat.finditer(text)]
        assert ref.starts(text.encode()) == starts, text
        table.append({"text": text, "starts": starts})
    # (b) the model
    corpus = [same_classes(synthetic(rng, rng.randint(3, 30))) for _ in range(3000)]
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.Sequence([pre_tokenizers.Split(Regex(ref.PATTERN), behavior="isolated", invert=False),
                                                 pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)])
    trainer = trainers.BpeTrainer(vocab_size=256 + 1 + 400, special_tokens=["<|end_of_text|>"], initial_alphabet=pre_tokenizers.ByteLevel.alphabet(),
                                  show_progress=False)
    tok.train_from_iterator(corpus, trainer)
    model_dir = os.path.join(gold, "pretok_cl100k")
    os.makedirs(model_dir, exist_ok=True)
    path = os.path.join(model_dir, "tokenizer.json")
    tok.save(path, pretty=False)
    words, ids, specials, name = batch.BPE.tokenizer_json_word_list(path)
    assert name == "cl100k" and specials == {"<|end_of_text|>": tok.token_to_id("<|end_of_text|>")} and len(words) == len(set(words)) > 400, (name, specials, len(words))
    d = bpe_ref.rank_dict(words)
    # (c) the texts
    texts = FIXED + [synthetic(rng, rng.randint(1, 12)) for _ in range(110)] + [ref.random_text(rng, 30) for _ in range(80)]
    cases = []
    for text in texts:
        same_classes(text)
        enc = tok.encode(text, add_special_tokens=False)
        blob = text.encode()
        char_of = []                       # the character that holds each byte
        for i, ch in enumerate(text):
            char_of += [i] * len(ch.encode())
        got_ids, got_off = [], []
        for a, e in ref.pretokens(blob):
            for pid, p0, p1 in bpe_ref.cut(blob[a:e], d, 4096, -1, ids):
                got_ids.append(pid)
                got_off.append([char_of[a + p0], char_of[a + p1 - 1] + 1])
        assert got_ids == list(enc.ids), (text, got_ids, enc.ids)
        assert got_off == [list(o) for o in enc.offsets], (text, got_off, enc.offsets)
        cases.append({"text": text, "ids": list(enc.ids), "offsets": [list(o) for o in enc.offsets]})
    for fname, doc in (("pretok_cl100k_worked.json", {"pattern": ref.PATTERN, "library": "regex " + regex.__version__, "cases": table}),
                       ("pretok_cl100k_cases.json", {"library": "tokenizers " + tokenizers.__version__,
                                                     "model": "models.BPE trained behind Sequence([Split(Regex(pattern), 'isolated'), ByteLevel(add_prefix_space=False, use_regex=False)])",
                                                     "offsets": "characters, as the package reports them: a piece covers every character it holds a byte of",
                                                     "cases": cases})):
        out = os.path.join(gold, fname)
        with open(out, "w", encoding="utf-8") as f:
            json.dump(doc, f, ensure_ascii=False, separators=(",", ":"))
            f.write("\n")
        print("%s: %d cases, %d bytes" % (out, len(doc["cases"]), os.path.getsize(out)))
    print("%s: %d words, %d bytes, %d pieces over %d texts" % (path, len(words), os.path.getsize(path), sum(len(c["ids"]) for c in cases), len(cases)))


if __name__ == "__main__":
    main()
