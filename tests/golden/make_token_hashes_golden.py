#!/usr/bin/env python3
"""Generate tests/golden/token_hashes.json (build container only: needs the reference tree and oracle/_ref).

DATA only: for every string of ref_strings.json and for the paragraph of c1_paragraph.json, the line itself, the tokens the REAL
reference produces -- tokenize(text) with its own latok.c and its own default_tokenizer.py (:149-160); an empty list where the
reference raises, i.e. for the empty string -- and, for two seeds, MurmurHash3 x86_32 of every token's UTF-8 bytes ("surrogatepass"),
computed by tests/helpers/murmur3_ref.py (held to the published vectors) and, where scikit-learn is installed, cross-checked
against sklearn.utils.murmurhash3_32.  tests/test_gpu_token_hashes.py replays it on the GPU box, where the reference does not exist.

Run:  make -C oracle ref && python3 tests/golden/make_token_hashes_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_loader  # noqa: E402
from helpers.murmur3_ref import VECTORS, murmur3_ref  # noqa: E402

SEEDS = (0, 0x9747B28C)


def main():
    assert all(murmur3_ref(d, s) == w for d, s, w in VECTORS)
    try:
        from sklearn.utils import murmurhash3_32 as sk
    except ImportError:
        sk = None
    dt = ref_loader.load_ref_python()
    items = json.load(open(os.path.join(HERE, "ref_strings.json")))["items"]
    lines = ["".join(map(chr, it["cps"])) for it in items]
    lines.append(json.load(open(os.path.join(HERE, "c1_paragraph.json")))["text"])
    tokens = []
    for text in lines:
        try:
            tokens.append([str(t) for t in dt.tokenize(text)])
        except Exception:
            assert text == "", text
            tokens.append([])
    hashes = {}
    for seed in SEEDS:
        rows = [[murmur3_ref(t.encode("utf-8", "surrogatepass"), seed) for t in toks] for toks in tokens]
        if sk is not None:
            assert rows == [[sk(t.encode("utf-8", "surrogatepass"), seed, positive=True) for t in toks] for toks in tokens]
        hashes[str(seed)] = rows
    with open(os.path.join(HERE, "token_hashes.json"), "w") as f:
        json.dump({"source": "real reference: tokenize(text); lines = ref_strings.json items in order, then c1_paragraph.json; "
                             "hashes[seed][line][k] = MurmurHash3 x86_32 of tokens[line][k] as UTF-8 (surrogatepass), as uint32",
                   "lines": lines, "tokens": tokens, "hashes": hashes}, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote token_hashes.json:", len(lines), "lines,", sum(map(len, tokens)), "tokens")


if __name__ == "__main__":
    main()
