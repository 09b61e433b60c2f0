#!/usr/bin/env python3
"""Generate tests/golden/join_tokens.json (build container only: needs the reference tree and oracle/_ref).

DATA only: for every string of ref_strings.json and for the paragraph of c1_paragraph.json, the line the REAL reference
produces -- " ".join(tokenize(text)) with its own latok.c and its own default_tokenizer.py (:149-160) -- (null would stand where the reference
raises, i.e. for the empty string; the present strings hold none).  tests/test_gpu_join_tokens.py replays it on the GPU box, where the reference does not exist.

Run:  make -C oracle ref && python3 tests/golden/make_join_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_loader  # noqa: E402


def main():
    dt = ref_loader.load_ref_python()
    items = json.load(open(os.path.join(HERE, "ref_strings.json")))["items"]
    texts = ["".join(map(chr, it["cps"])) for it in items]
    texts.append(json.load(open(os.path.join(HERE, "c1_paragraph.json")))["text"])
    rows = []
    for text in texts:
        try:
            rows.append(" ".join(dt.tokenize(text)))
        except Exception:
            assert text == "", text
            rows.append(None)
    with open(os.path.join(HERE, "join_tokens.json"), "w") as f:
        json.dump({"source": "real reference: ' '.join(tokenize(text)); strings = ref_strings.json items in order, then c1_paragraph.json",
                   "sep": " ", "rows": rows}, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote join_tokens.json:", len(rows), "rows,", sum(r is None for r in rows), "null")


if __name__ == "__main__":
    main()
