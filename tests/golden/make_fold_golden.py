#!/usr/bin/env python3
"""Generate tests/golden/fold_map.json from this interpreter's own str.lower() and unicodedata: the data behind
latok_fold_utf8_bytes_batch (include/latok_hip.h) as tests/helpers/fold_ref.py reads it.

* ``unidata_version``: the UCD version of the interpreter that wrote the file;
* ``map``: for every non-Hangul code point whose LOWER or STRIP_MARKS image differs from itself, ``[c, lower_seq, strip_seq]``
  (lower_seq = the code points of chr(c).lower(); strip_seq = those of NFD(chr(c)) whose category is not Mn);
* ``cc_cf`` / ``zs``: the code points of category Cc or Cf / Zs as inclusive ranges.

Hangul syllables (arithmetic) and the CJK ranges are not in the file.  tests/test_fold_host.py repeats the sweep and compares where
the interpreter's UCD version is the file's."""
import json
import os
import unicodedata as ud

HERE = os.path.dirname(os.path.abspath(__file__))
S_BASE, S_COUNT = 0xAC00, 11172


def ranges(cps):
    out = []
    for c in cps:
        if out and out[-1][1] == c - 1:
            out[-1][1] = c
        else:
            out.append([c, c])
    return out


def sweep():
    rows, cc_cf, zs = [], [], []
    for c in range(0x110000):
        ch = chr(c)
        cat = ud.category(ch)
        if cat in ("Cc", "Cf"):
            cc_cf.append(c)
        elif cat == "Zs":
            zs.append(c)
        if S_BASE <= c < S_BASE + S_COUNT:
            continue
        lower = [ord(x) for x in ch.lower()]
        strip = [ord(x) for x in ud.normalize("NFD", ch) if ud.category(x) != "Mn"]
        if lower != [c] or strip != [c]:
            rows.append([c, lower, strip])
    return {"unidata_version": ud.unidata_version, "map": rows, "cc_cf": ranges(cc_cf), "zs": ranges(zs)}


if __name__ == "__main__":
    g = sweep()
    with open(os.path.join(HERE, "fold_map.json"), "w") as f:
        json.dump(g, f, separators=(",", ":"))
        f.write("\n")
    print("wrote fold_map.json: UCD %s, %d rows, %d Cc/Cf ranges, %d Zs ranges" % (g["unidata_version"], len(g["map"]), len(g["cc_cf"]), len(g["zs"])))
