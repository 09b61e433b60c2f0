#!/usr/bin/env python3
"""Makes the fixtures of the SentencePiece BPE tests (tests/golden/spbpe/): trains a small BPE model with the ``sentencepiece`` package
from a seeded corpus generated here, spells the same model as a Hugging Face ``tokenizer.json`` with the ``tokenizers`` package, and
records what the two packages give for a seeded list of texts.  Needs both packages; the tests need neither.

    m.model            the trained model (byte_fallback, identity normalizer, dummy prefix, whitespace kept)
    tokenizer.json     the same vocabulary as models.BPE with merges derived from the pieces, Prepend + Replace as normalizer
    spbpe_cases.json   {"cases": [{"text", "sp_ids", "hf_ids", "hf_offsets"}]}: SentencePieceProcessor.encode, Tokenizer.encode
    spbpe_worked.json  {"cases": [{"text", "segments"}]}: segment tables worked by hand (below), checked against the reference here

Before anything is written the built-in reader of the model file (latok_amd.batch.BPE.read_sentencepiece_model) is compared with the
package's own parse, and tests/helpers/spbpe_ref.py with both packages on every case: a disagreement stops the tool."""
import io
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MARK = "▁"
WORDS = ["the", "quick", "brown", "fox", "jumps", "over", "lazy", "dog", "hello", "world", "token", "tokens", "model", "models", "naïve",
         "café", "straße", "日本語", "テスト", "привет", "мир", "ab", "abc", "abcd", "x", "y", "z", "1", "22", "333", "don't", "e-mail", "a.b",
         "(paren)", "new\nline", "tab\tbed"]

# segment tables worked by hand: text -> the segments, which join back to the text
WORKED = [
    ("", []),
    (" ", [" "]),
    ("a", ["a"]),
    ("a b", ["a", " b"]),
    ("a  b", ["a", "  b"]),
    (" a", [" a"]),
    ("  a ", ["  a", " "]),
    ("a ", ["a", " "]),
    ("   ", ["   "]),
    ("a" + MARK + "b", ["a", MARK + "b"]),
    ("a" + MARK + " b", ["a", MARK + " b"]),
    ("a " + MARK + " " + MARK + "b c", ["a", " " + MARK + " " + MARK + "b", " c"]),
    (MARK + MARK, [MARK + MARK]),
    ("a\tb c\nd", ["a\tb", " c\nd"]),
    ("\t a", ["\t", " a"]),
    ("日本 語", ["日本", " 語"]),
    ("a\u00a0b c", ["a\u00a0b", " c"]),          # (U+00A0 is an ordinary character)
    ("x" + MARK, ["x", MARK]),
    ("hello  world  ", ["hello", "  world", "  "]),
    (" \n ", [" \n", " "]),
]


def corpus(rng):
    lines = []
    for _ in range(4000):
        n = rng.randint(1, 9)
        parts = []
        for _ in range(n):
            parts.append(rng.choice(WORDS))
            parts.append(rng.choice([" ", " ", " ", " ", "  ", "   ", "    "]))
        lines.append("".join(parts[:-1]) + rng.choice(["", "", " ", "."]))
    return lines


def case_texts(rng):
    edge = ["", " ", "  ", "a", "a  b", "a" + MARK + " b", " a", "a ", MARK, MARK + MARK + "x", "hello world", "  hello   world  ", "\t", "\n\n",
            "a\tb", "😀", "a😀b", " 😀 ", "日本語 テスト", "q", "qq qq", "the quick brown fox jumps over the lazy dog", "x" * 40, " " * 9,
            "ab abc abcd", "don't", "naïve café", "ÿ", "€", "a€ b", "привет мир", MARK + " " + MARK, "tokens" * 8, "a" + " " * 5 + "b"]
    alphabet = list("abcdehlnorstwxyz") + [" "] * 8 + ["  ", "\t", "\n", "é", "ï", "ß", "日", "本", "語", "€", "😀", "𝒳", MARK, "п", "1", ".", "'"]
    out = list(edge)
    for _ in range(120):
        out.append("".join(rng.choice(alphabet) for _ in range(rng.randint(1, 40))))
    for _ in range(80):
        n = rng.randint(1, 8)
        out.append("".join(rng.choice(WORDS) + rng.choice([" ", " ", "  ", "   ", "", "\n"]) for _ in range(n)))
    return out


def derive_merges(pieces):
    """the merges of a tokenizer.json from the NORMAL pieces in id order (which is score order): every split of a piece into two pieces of
    the vocabulary, the splits of one piece ordered by the ids of their halves"""
    vocab = {p: i for i, (p, _s, _t) in enumerate(pieces)}
    merges = []
    for i, (p, _s, t) in enumerate(pieces):
        if t != 1 or len(p) < 2:
            continue
        local = [(vocab[p[:k]], vocab[p[k:]], p[:k], p[k:]) for k in range(1, len(p)) if p[:k] in vocab and p[k:] in vocab]
        merges += [(l, r) for _a, _b, l, r in sorted(local)]
    return vocab, merges


def main():
    import sentencepiece as spm
    from sentencepiece import sentencepiece_model_pb2 as pb2
    from tokenizers import Tokenizer, models, normalizers
    from helpers import spbpe_ref as ref
    from latok_amd.batch import BPE

    out_dir = os.path.join(ROOT, "tests", "golden", "spbpe")
    os.makedirs(out_dir, exist_ok=True)
    rng = random.Random(20240917)
    blob = io.BytesIO()
    spm.SentencePieceTrainer.train(sentence_iterator=iter(corpus(rng)), model_writer=blob, vocab_size=400, model_type="bpe", byte_fallback=True,
                                   normalization_rule_name="identity", add_dummy_prefix=True, remove_extra_whitespaces=False,
                                   allow_whitespace_only_pieces=True, character_coverage=0.995, num_threads=1, minloglevel=2)
    model_path = os.path.join(out_dir, "m.model")
    with open(model_path, "wb") as f:
        f.write(blob.getvalue())

    # the built-in reader against the package's own parse
    proto = pb2.ModelProto()
    proto.ParseFromString(blob.getvalue())
    mine = BPE.read_sentencepiece_model(model_path)
    assert [(p.piece.encode(), p.score, p.type) for p in proto.pieces] == mine["pieces"]
    ts, ns = proto.trainer_spec, proto.normalizer_spec
    assert (ts.model_type, ts.byte_fallback, ts.treat_whitespace_as_suffix) == (mine["model_type"], mine["byte_fallback"], mine["treat_whitespace_as_suffix"])
    assert (ns.name, ns.precompiled_charsmap, ns.add_dummy_prefix, ns.remove_extra_whitespaces, ns.escape_whitespaces) == (
        mine["normalizer_name"], mine["charsmap"], mine["add_dummy_prefix"], mine["remove_extra_whitespaces"], mine["escape_whitespaces"])

    # the same model as a tokenizer.json
    pieces = [(p.piece, p.score, p.type) for p in proto.pieces]
    vocab, merges = derive_merges(pieces)
    tok = Tokenizer(models.BPE(vocab, merges, byte_fallback=True, fuse_unk=True, unk_token="<unk>"))
    tok.normalizer = normalizers.Sequence([normalizers.Prepend(MARK), normalizers.Replace(" ", MARK)])
    tok.add_special_tokens([p for p, _s, t in pieces if t in (2, 3)])
    json_path = os.path.join(out_dir, "tokenizer.json")
    tok.save(json_path)

    sp = spm.SentencePieceProcessor(model_file=model_path)
    words, ids, byte_ids, _specials, dummy = BPE.sentencepiece_word_list(model_path)
    d = ref.rank_dict(words)
    jw, jids, jbytes, _js, jdummy = BPE.spm_tokenizer_json_word_list(json_path)
    jd = ref.rank_dict(jw)
    cases = []
    for text in case_texts(rng):
        sp_ids = [int(i) for i in sp.encode(text)]
        enc = tok.encode(text, add_special_tokens=False) if text else None
        hf_ids = list(enc.ids) if enc else []
        hf_offsets = [list(o) for o in enc.offsets] if enc else []
        got, _spans = ref.encode(text.encode(), d, byte_ids=byte_ids, ids=ids, add_dummy_prefix=dummy)
        got_j, _spans = ref.encode(text.encode(), jd, byte_ids=jbytes, ids=jids, add_dummy_prefix=jdummy)
        assert got == sp_ids, (text, got, sp_ids)
        assert got_j == hf_ids == sp_ids, (text, got_j, hf_ids, sp_ids)
        cases.append(dict(text=text, sp_ids=sp_ids, hf_ids=hf_ids, hf_offsets=hf_offsets))
    assert len(cases) >= 200
    with open(os.path.join(out_dir, "spbpe_cases.json"), "w", encoding="utf-8") as f:
        json.dump(dict(sentencepiece=spm.__version__, cases=cases), f, ensure_ascii=False, indent=0)

    worked = []
    for text, segs in WORKED:
        b = text.encode()
        assert "".join(segs) == text
        assert [b[a:e] for a, e in ref.segments(b)] == [s.encode() for s in segs], text
        worked.append(dict(text=text, segments=segs))
    with open(os.path.join(out_dir, "spbpe_worked.json"), "w", encoding="utf-8") as f:
        json.dump(dict(cases=worked), f, ensure_ascii=False, indent=0)
    print("wrote %d cases, %d worked tables, %d pieces, %d merges" % (len(cases), len(worked), len(pieces), len(merges)))


if __name__ == "__main__":
    main()
