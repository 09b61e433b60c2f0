"""Child process of tests/test_gpu_span_strip.py::test_chunked_host_pipeline: the `mid` content of every table through the chunked
host pipeline (LATOK_PIPE_CHUNK_CHARS is set small by the parent and read once by the library), compared in full with the reference.
usage: span_strip_pipeline_child.py <repository root>"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = sys.argv[1]
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "helpers")]
import latok_oracle as oracle  # noqa: E402
import span_strip_content as ssc  # noqa: E402
from conftest import pack  # noqa: E402
from latok_amd import _lib, batch  # noqa: E402

CHUNK = int(os.environ["LATOK_PIPE_CHUNK_CHARS"])
last_plan = _lib.load().latok_debug_last_plan
last_plan.restype, last_plan.argtypes = C.c_int, [C.c_void_p, C.c_int]


def chunked(total):
    """the last tile pipeline of the call covered less than the batch: it ran chunk by chunk"""
    out = np.zeros(15, np.int64)
    assert last_plan(out.ctypes.data, 15) == 15
    return total >= 2 * CHUNK and out[14] < (total + ssc.TILE - 1) // ssc.TILE


reached = set()
for table in sorted(ssc.TABLES):
    batch.set_rules(*ssc.TABLES[table])
    try:
        for form, kind, rg in (("utf32", 4, "full"), ("kind1", 1, "latin1"), ("kind2", 2, "bmp")):
            for i, texts in enumerate(ssc.content(table, "mid", "chars", rg)[:3]):
                r = ssc.reference(oracle, texts, ssc.TABLES[table], "chars")
                cps, row = pack(texts)
                units = cps if kind == 4 else cps.astype(np.uint8 if kind == 1 else np.uint16)
                for dt in (np.int64, np.int32):
                    for feats in (False, True):
                        if kind == 4:
                            got = (batch.token_features_csr if feats else batch.token_spans_csr)(units, row, dtype=dt)
                        else:
                            got = (batch.token_features_kind_csr if feats else batch.token_spans_kind_csr)(units, row, dtype=dt)
                        assert chunked(r.total), (table, form, i, r.total)
                        ssc.compare(got, r, dt, feats, (table, form, "pipeline", "ABC"[i], dt.__name__, feats))
                reached.add(form)
        for i, texts in enumerate(ssc.content(table, "mid", "bytes")[:3]):      # byte space: spans (featurize has a route of its own)
            r = ssc.reference(oracle, texts, ssc.TABLES[table], "bytes")
            u8, boff = batch.pack_utf8([t.encode("utf-8") for t in texts])
            for dt in (np.int64, np.int32):
                got = batch.token_spans_utf8_bytes_csr(u8, boff, dtype=dt)
                assert chunked(r.total), (table, "utf8_bytes", i, r.total)
                ssc.compare(got, r, dt, False, (table, "utf8_bytes", "pipeline", "ABC"[i], dt.__name__))
            reached.add("utf8_bytes")
    finally:
        batch.reset_rules()
for form in sorted(reached):
    print("reached", form)
print("ok")
