"""Every entry-point family after every other on ONE context (include/latok_hip.h).

A context owns one set of device workspaces, eight pinned total words, one chained-scan state, one host staging area and one stream-turn
event, and 35 entry-point families share them.  Each family's own tests run it first or alone on its context; here the families follow
each other in plans that put every ordered pair side by side (helpers/call_sequences.pair_cover), every family behind every refused
call (after_each), the boundary families behind set_rules / reset_rules, every pair on rotating caller streams, and the multi-scan
families across the wrap of the scan epoch.  Batches alternate between a DENSE and a SPARSE content of the sizes E, S, S600, SN, M, M5, L
(thresholds from latok_debug_limits and LATOK_TILE_CHARS), so that a short sparse batch regularly meets planes, keys and rows the batch
before it left full.

Every expectation is independent of the library: boundaries and feature columns from the oracle, decode from helpers/utf8_ref.py, fold
from helpers/fold_ref.py, hashes from helpers/murmur3_ref.py, WordPiece from helpers/wordpiece_ref.py, TF-IDF from helpers/tfidf_ref.py
under the header's bounds, term / n-gram / counter results from collections.Counter over the reference tokens.  Integer and byte outputs
are compared exactly and in full; every output buffer ends in 64 poison elements that must survive; the output width is int64 on a
family's even occurrences and LATOK_OUT_INT32 on its odd ones.  tests/test_call_sequences_host.py shows that the driver sees an
order-dependent error.

Ten families came after those 35: character n-grams inside tokens (vocabulary and hashed), byte-level BPE (ids on latok's tokens, ids on
GPT-2's pre-tokens, padded), the pre-tokens themselves, Unigram (ids, padded) and decoding (CSR, padded).  They stand beside the 35 in
plans of their own: every ordered pair that has one of the ten in it (helpers/call_sequences.pair_cover_touching), every family behind
every refusal of the ten and the ten behind every refusal of the 35, the rule tables in front of the ten, the touching plan on rotating
caller streams, the epoch wrap inside their multi-scan calls.  Their expectations come from helpers/bpe_ref.py, unigram_ref.py,
pretok_ref.py, chargram_ref.py and detok_ref.py over the reference tokens, and their word lists are built here without the library."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import RULE_SETS
from helpers import bpe_ref
from helpers import call_sequences as cs
from helpers import chargram_ref
from helpers import detok_ref
from helpers import fold_ref
from helpers import pretok_ref
from helpers import tfidf_ref
from helpers import unigram_ref
from helpers import utf8_ref
from helpers import wordpiece_ref as wpr
from helpers.murmur3_ref import murmur3_ref

pytestmark = pytest.mark.gpu

GUARD, POISON = 64, 0xA5
SEED, NC = 0x9747B28C, 128                       # hash seed; columns of both idf objects = n_features of the hashed forms
UNK, WP_UNK, WP_CLS, WP_SEP, WP_PAD, WP_LEN = -7, 1, 2, 3, 0, 12
MATRIX_CHARS = 700
VOCAB = {w: i for i, w in reversed(list(enumerate(cs.VOCAB_WORDS)))}       # of a duplicate word the first wins
WP_DICT = wpr.vocab_dict(cs.WP_WORDS)
FROZEN_DF = np.array([(c * 5) % 9 for c in range(NC)], np.int32)
FROZEN_DOCS = 8
NORMS = {"E": "l2", "S": "l1", "S600": None, "SN": "l2", "M": "l2", "M5": "l1", "L": None}
NORM_BIT = {"l1": 4, "l2": 8, None: 0}
C_SPLIT = np.array([[5, -1], [6, -1], [20, -1], [4, 17], [4, 16]], np.int8)
C_MASK = np.array([[7, 18, 13, -1], [11, 18, 21, 23], [8, 14, 15, -1], [9, 22, 24, 12]], np.int8)


@functools.lru_cache(maxsize=1)
def _limits():
    """(LATOK_TILE_CHARS, kSmallChars, kSmallStrings)"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    lim = np.zeros(8, np.int64)
    assert fn(lim.ctypes.data, 8) == 8 and lim[0] == _lib.TILE_CHARS
    return int(_lib.TILE_CHARS), int(lim[6]), int(lim[7])


@functools.lru_cache(maxsize=1)
def _batches():
    tile, small_chars, small_strings = _limits()
    return cs.build_batches(tile, small_chars, small_strings)


@functools.lru_cache(maxsize=None)
def _hash(token):
    return murmur3_ref(token, SEED)


# ---- the context's objects, buffers and state ---------------------------------------------------------------------------------------
class Out:
    """an output buffer of n elements and GUARD more, all poison; on the device in device mode"""

    def __init__(self, env, n, dtype, tail=()):
        self.env = env
        self.h = np.empty((max(int(n), 0) + GUARD,) + tuple(tail), dtype)
        self.h.reshape(-1).view(np.uint8)[:] = POISON
        self.ptr = env.alloc(self.h.nbytes, self.h) if env.device else self.h.ctypes.data

    def read(self, valid):
        """(the first ``valid`` elements, the number of bytes behind them that are no longer poison)"""
        if self.env.device:
            self.env.d2h(self.h, self.ptr)
        rest = self.h[valid:].reshape(-1).view(np.uint8)
        return self.h[:valid].copy(), int(np.count_nonzero(rest != POISON))


def P(out):
    return None if out is None else out.ptr


class Env:
    """One context's worth of test state: the library, the pointer mode, the device objects, the plain-Python accumulation of what the
    counter and the accumulating idf have seen, the device copies of the inputs and the caller streams."""

    def __init__(self, lib, oracle, device):
        from latok_amd import _lib, batch
        self.lib, self.oracle, self.device, self._lib = lib, oracle, device, _lib
        self.acc_df, self.acc_docs = np.zeros(NC, np.int64), 0
        self.acc_words, self.acc_tokens = {}, 0
        self.inputs, self.live, self.holds, self.keep, self.kept = {}, [], [], False, []
        self.streams, self.calls, self.defer, self.rules = None, 0, False, None
        if lib is None:
            return                                     # expectations only (tests/test_call_sequences_host.py): no device object
        self.vocab = batch.Vocab(cs.VOCAB_WORDS)
        bad_ids = np.arange(len(cs.VOCAB_WORDS))
        for w in (b"a", b"a b"):                                            # a term and a gram of every dense batch: a column no idf
            bad_ids[VOCAB[w]] = NC + 5                                      # of NC columns has
        self.vocab_bad = batch.Vocab(cs.VOCAB_WORDS, bad_ids)
        self.wp = batch.WordPiece(cs.WP_WORDS, prefix=cs.WP_PREFIX, max_chars=100)
        self.counter = batch.TokenCounter(1 << 14, 256, seed=SEED)
        self.idf_acc, self.idf_frozen = batch.Idf(NC), batch.Idf(NC)
        self.idf_frozen.load(FROZEN_DF, FROZEN_DOCS)
        # the objects of the ten later families (their word lists: below, beside the families)
        self.cg_vocab = batch.Vocab(CG_WORDS)
        self.bpe = batch.BPE(BPE_WORDS, max_bytes=PIECE_MAX_BYTES, lead_space=True)
        self.bpe_gpt2 = batch.BPE(GPT2_WORDS, max_bytes=PIECE_MAX_BYTES, lead_space=False, pretokenizer="gpt2")
        self.uni = batch.Unigram(UNI_WORDS, UNI_SCORES, marker=unigram_ref.MARKER, unk_score=UNI_UNK_SCORE, fuse_unk=True, max_bytes=PIECE_MAX_BYTES)
        self.detok_bpe = batch.Detokenizer(BPE_WORDS, mode="concat")
        self.detok_wp = batch.Detokenizer(cs.WP_WORDS, mode="wordpiece", prefix=cs.WP_PREFIX, sep=b" ")

    def close(self):
        self.release(self.kept)
        for p, _ in self.inputs.values():
            if self.device:
                self.lib.latok_dev_free(p)
        for o in (self.vocab, self.vocab_bad, self.wp, self.counter, self.idf_acc, self.idf_frozen, self.cg_vocab, self.bpe, self.bpe_gpt2, self.uni,
                  self.detok_bpe, self.detok_wp):
            o.close()

    # -- memory
    def alloc(self, nbytes, fill=None):
        p = self.lib.latok_dev_alloc(nbytes + 64)
        assert p, "device allocation failed"
        if fill is not None and fill.nbytes:
            self._lib.check(self.lib.latok_memcpy_h2d(p, fill.ctypes.data, fill.nbytes))
        self.live.append(p)
        return p

    def begin(self):
        self.live, self.holds = [], []
        return self.live

    def release(self, live):
        if self.keep and live is not self.kept:
            self.kept += live
        else:
            for p in live:
                self.lib.latok_dev_free(p)
        del live[:]

    def d2h(self, arr, p):
        if arr.nbytes:
            self._lib.check(self.lib.latok_memcpy_d2h(arr.ctypes.data, p, arr.nbytes))

    def inp(self, arr, cache=True):
        """pointer to an input array: the array itself (padded by 64 bytes) or its device copy"""
        arr = np.ascontiguousarray(arr)
        if not cache:
            if self.device:
                return self.alloc(arr.nbytes, arr)
            pad = np.concatenate([arr.reshape(-1).view(np.uint8), np.zeros(64, np.uint8)])
            self.holds.append(pad)                     # (a host-pointer call is over when it returns)
            return pad.ctypes.data
        k = id(arr)
        if k not in self.inputs or self.inputs[k][1] is not arr:
            if self.device:
                live, self.live = self.live, []
                p = self.alloc(arr.nbytes, arr)
                self.live = live
                self.inputs[k] = (p, arr)
            else:
                pad = np.concatenate([arr.reshape(-1).view(np.uint8), np.zeros(64, np.uint8)])
                self.inputs[k] = (pad, arr)
        e = self.inputs[k][0]
        return e if self.device else e.ctypes.data

    def upload_all(self, batches):
        """device mode: every input form of every batch in device memory before the first call"""
        for b in batches.values():
            for a in (b.u8, b.boff, b.cps, b.row, b.k1, b.k2):
                self.inp(a)
        self._lib.check(self.lib.latok_sync())

    # -- streams
    def next_stream(self):
        s = self.streams[self.calls % len(self.streams)] if self.streams else None
        self.calls += 1
        return s

    def sync(self, stream):
        if not self.device:
            return
        if stream is None:
            self._lib.check(self.lib.latok_sync())
        else:
            assert self.lib.hipStreamSynchronize(stream) == 0

    # -- references and state
    def ref(self, b, form="cps"):
        if self.rules is None:
            return cs.reference(self.oracle, b, None, form)
        return cs.reference(self.oracle, b, RULE_SETS[self.rules], form, self.rules)

    def state(self):
        """what the counter and the accumulating idf hold now, read from the device"""
        st = np.zeros(5, np.int64)
        self._lib.check(self.lib.latok_counter_info(self.counter.handle, None, None, None, None, None, st.ctypes.data))
        df, n_docs = np.full(NC, -1, np.int32), C.c_int64(-1)
        self._lib.check(self.lib.latok_idf_read(self.idf_acc.handle, df.ctypes.data, NC, C.byref(n_docs)))
        return {"state: counter stats5": st, "state: idf df": df, "state: idf n_docs": np.array([n_docs.value])}

    def want_state(self):
        n = sum(self.acc_words.values())
        return {"state: counter stats5": np.array([self.acc_tokens, n, self.acc_tokens - n, 0, len(self.acc_words)], np.int64),
                "state: idf df": self.acc_df.copy(), "state: idf n_docs": np.array([self.acc_docs])}


# ---- the family base ----------------------------------------------------------------------------------------------------------------
class Fam:
    """One entry point.  ``mode``: "fit" (exact capacity; the call succeeds), "short" (capacity one short), "query" (capacity 0, no record
    buffers), "decreasing" (a row offset that decreases; host pointers), "badcol" (a column no idf has).  run() makes the call and returns
    (rc, [(name, Out, valid elements)], {scalar name: value}); full() is the reference of the successful call."""
    uses_l = stateful_family = asynchronous = boundary = False
    has_width = True
    records, modes = (), ("fit",)
    entry = None

    def __init__(self, env, mode="fit"):
        self.env, self.mode, self.occ, self.odd = env, mode, 0, 0
        self.name = self.entry + ("" if mode == "fit" else "[%s]" % mode)
        self._full = {}

    @property
    def stateful(self):
        """whether the expectation depends on more than (family, batch, width): on what the objects have seen, or on the rules"""
        return self.stateful_family or self.mode != "fit" or self.env.rules is not None

    # helpers for run()
    @property
    def dt(self):
        return np.int32 if (self.odd and self.has_width) else np.int64

    @property
    def flags(self):
        _lib = self.env._lib
        return (_lib.DEVICE_PTRS if self.env.device else 0) | (_lib.OUT_INT32 if (self.odd and self.has_width) else 0)

    def out(self, n, dtype, tail=()):
        return Out(self.env, n, dtype, tail)

    def cap(self, need):
        return {"short": need - 1, "query": 0}.get(self.mode, need)

    def rec(self, need, dtype, tail=()):
        return None if self.mode == "query" else Out(self.env, self.cap(need), dtype, tail)

    def offs(self, arr):
        """the offsets array as the call gets it: in "decreasing" mode one entry lies above its successor"""
        if self.mode != "decreasing":
            return self.env.inp(arr)
        c = arr.copy()
        i = (c.size - 1) // 2
        assert c.size >= 3
        c[i] = c[i + 1] + 1
        return self.env.inp(c, cache=False)

    def cached(self, b):
        k = (b.key, self.odd, self.env.rules)
        if k not in self._full:
            self._full[k] = self.full(b)
        return self._full[k]

    # the two methods the driver uses
    def call(self, b, occ):
        env = self.env
        self.occ, self.odd = occ, occ % 2
        live = env.begin()
        self.stream = env.next_stream()
        stream, mode = self.stream, self.mode
        rc, outs, scalars = self.run(b)

        def resolve():
            env.sync(stream)
            res, damage = {"rc": np.array([rc])}, 0
            for name, out, valid in outs:
                if out is None:
                    continue
                if mode in ("decreasing", "badcol") or rc != (0 if mode == "fit" else -1) or (mode == "short" and name in self.records):
                    valid = 0
                arr, bad = out.read(valid)
                res[name], damage = arr, damage + bad
            res["guard bytes overwritten"] = np.array([damage])
            if mode in ("fit", "short", "query"):
                res.update({k: np.array([v]) for k, v in scalars.items()})
            if mode != "fit":
                res.update(env.state())
            env.release(live)
            return res

        return resolve if (env.defer and self.asynchronous and mode == "fit") else resolve()

    def expect(self, b):
        full = self.full(b) if self.stateful_family else self.cached(b)
        want = {"rc": np.array([0 if self.mode == "fit" else -1]), "guard bytes overwritten": np.array([0])}
        for name, v in full.items():
            scalar = np.ndim(v) == 0 and not isinstance(v, cs.Approx)
            if self.mode == "fit":
                want[name] = np.array([v]) if scalar else v
            elif scalar:
                if self.mode in ("short", "query"):
                    want[name] = np.array([v])
            elif self.mode == "query" and name in self.records:
                continue
            elif self.mode in ("decreasing", "badcol") or name in self.records:
                w = v.want if isinstance(v, cs.Approx) else v
                want[name] = np.zeros((0,) + w.shape[1:], np.float32 if isinstance(v, cs.Approx) else w.dtype)
            else:
                want[name] = v
        if self.mode != "fit":
            want.update(self.env.want_state())
        return want


CAP_MODES = ("fit", "short", "query", "decreasing")


# ---- UTF-32, PEP 393 kinds, code-point UTF-8, byte space: masks and compaction ------------------------------------------------------
class Mask(Fam):
    """latok_split_mask_batch / latok_split_values_batch / latok_split_mask_utf8_bytes_batch"""
    asynchronous = boundary = True
    has_width = False
    modes = ("fit", "decreasing")

    def __init__(self, env, mode, entry, form, attr, dtype, uses_l):
        self.entry, self.form, self.attr, self.dtype, self.uses_l = entry, form, attr, dtype, uses_l
        super().__init__(env, mode)

    def full(self, b):
        return {"out": getattr(self.env.ref(b), self.attr)}

    def run(self, b):
        data, off, total = (b.cps, b.row, b.total_chars) if self.form == "cps" else (b.u8, b.boff, b.total_bytes)
        n = total if self.dtype == np.uint8 else (total + 63) // 64
        o = self.out(n, self.dtype)
        rc = getattr(self.env.lib, self.entry)(self.env.inp(data), self.offs(off), b.n_str, total, o.ptr, self.flags, self.stream)
        return rc, [("out", o, n)], {}


class Compact(Fam):
    """offsets / spans / features of every input form: counts, records (and sums), the total"""
    boundary = True
    records, modes = ("items", "feats"), CAP_MODES

    def __init__(self, env, mode, entry, form, what, uses_l):
        self.entry, self.form, self.what, self.uses_l = entry, form, what, uses_l
        super().__init__(env, mode)

    def full(self, b):
        r = self.env.ref(b, self.form if self.form in ("k1", "k2") else "cps")
        byte = self.form == "bytes"
        if self.what == "offsets":
            return {"counts": r.off_counts, "items": r.byte_offsets if byte else r.offsets, "n": int(r.off_counts.sum())}
        if self.what == "spans":
            return {"counts": r.counts, "items": r.byte_spans if byte else r.spans, "n": r.n_tokens}
        return {"counts": r.counts, "items": r.byte_spans4 if byte else r.spans4, "feats": r.feats, "n": r.n_tokens}

    def run(self, b):
        env = self.env
        data, off, total = {"cps": (b.cps, b.row, b.total_chars), "k1": (b.k1, b.row, b.total_chars), "k2": (b.k2, b.row, b.total_chars),
                            "u8": (b.u8, b.boff, b.total_bytes), "bytes": (b.u8, b.boff, b.total_bytes)}[self.form]
        need = self.cached(b)["n"]
        tail = {"offsets": (), "spans": (2,), "features": (4,)}[self.what]
        counts, items = self.out(b.n_str, self.dt), self.rec(need, self.dt, tail)
        feats = self.rec(need, np.int8, (25,)) if self.what == "features" else None
        n = C.c_int64(-1)
        args = [env.inp(data)] + ([int(self.form[1])] if self.form in ("k1", "k2") else []) + [self.offs(off), b.n_str, total, counts.ptr, P(items)]
        args += ([P(feats)] if self.what == "features" else []) + [self.cap(need), C.byref(n), self.flags, self.stream]
        rc = getattr(env.lib, self.entry)(*args)
        return rc, [("counts", counts, b.n_str), ("items", items, need), ("feats", feats, need)], {"n": n.value}


class Decode(Fam):
    entry, uses_l, has_width = "latok_utf8_decode_batch", True, False
    records, modes = ("cps", "cp_row"), ("fit", "short", "decreasing")

    def full(self, b):
        cps, row, total = utf8_ref.decode_batch(b.u8, b.boff)
        return {"cps": cps, "cp_row": row, "total_cps": total}

    def run(self, b):
        need = b.total_chars
        cps, row, n = self.rec(need, np.uint32), self.out(b.n_str + 1, np.int64), C.c_int64(-1)
        rc = self.env.lib.latok_utf8_decode_batch(self.env.inp(b.u8), self.offs(b.boff), b.n_str, b.total_bytes, P(cps), self.cap(need), row.ptr,
                                                  C.byref(n), self.flags, self.stream)
        return rc, [("cps", cps, need), ("cp_row", row, b.n_str + 1)], {"total_cps": n.value}


class MaskUtf8(Fam):
    entry, uses_l, has_width, boundary = "latok_split_mask_utf8_batch", True, False, True
    records, modes = ("mask", "cp_row"), ("fit", "short", "decreasing")

    def full(self, b):
        return {"mask": self.env.ref(b).cp_mask, "cp_row": b.row, "total_cps": b.total_chars}

    def run(self, b):
        need = (b.total_chars + 63) // 64
        mask, row, n = self.rec(need, np.uint64), self.out(b.n_str + 1, np.int64), C.c_int64(-1)
        rc = self.env.lib.latok_split_mask_utf8_batch(self.env.inp(b.u8), self.offs(b.boff), b.n_str, b.total_bytes, P(mask), self.cap(need), row.ptr,
                                                      C.byref(n), self.flags, self.stream)
        return rc, [("mask", mask, need), ("cp_row", row, b.n_str + 1)], {"total_cps": n.value}


# ---- byte space: text, hashes, ids ---------------------------------------------------------------------------------------------------
class Join(Fam):
    entry, records, modes = "latok_join_tokens_utf8_bytes_batch", ("bytes",), CAP_MODES
    SEP = 0x2C

    def full(self, b):
        r = self.env.ref(b)
        out, off = r.join(self.SEP)
        return {"bytes": out, "out_off": off, "counts": r.counts, "n": int(off[-1])}

    def run(self, b):
        need = self.cached(b)["n"]
        out, off, counts, n = self.rec(need, np.uint8), self.out(b.n_str + 1, np.int64), self.out(b.n_str, self.dt), C.c_int64(-1)
        rc = self.env.lib.latok_join_tokens_utf8_bytes_batch(self.env.inp(b.u8), self.offs(b.boff), b.n_str, b.total_bytes, self.SEP, P(out),
                                                             self.cap(need), off.ptr, counts.ptr, C.byref(n), self.flags, self.stream)
        return rc, [("bytes", out, need), ("out_off", off, b.n_str + 1), ("counts", counts, b.n_str)], {"n": n.value}


class HashesIds(Fam):
    """latok_token_hashes_utf8_bytes_batch / latok_token_ids_utf8_bytes_batch"""
    records, modes = ("spans", "values"), CAP_MODES

    def __init__(self, env, mode, ids):
        self.ids, self.entry = ids, "latok_token_ids_utf8_bytes_batch" if ids else "latok_token_hashes_utf8_bytes_batch"
        super().__init__(env, mode)

    def full(self, b):
        r = self.env.ref(b)
        v = np.array([VOCAB.get(t, UNK) for t in r.tokens], np.int32) if self.ids else np.array([_hash(t) for t in r.tokens], np.uint32)
        return {"counts": r.counts, "spans": r.byte_spans, "values": v, "n": r.n_tokens}

    def run(self, b):
        env, need = self.env, self.cached(b)["n"]
        counts, spans = self.out(b.n_str, self.dt), self.rec(need, self.dt, (2,))
        vals, n = self.rec(need, np.int32 if self.ids else np.uint32), C.c_int64(-1)
        head = [env.inp(b.u8), self.offs(b.boff), b.n_str, b.total_bytes] + ([env.vocab.handle, UNK] if self.ids else [SEED])
        rc = getattr(env.lib, self.entry)(*head, counts.ptr, P(spans), P(vals), self.cap(need), C.byref(n), self.flags, self.stream)
        return rc, [("counts", counts, b.n_str), ("spans", spans, need), ("values", vals, need)], {"n": n.value}


# ---- byte space: term counts, n-grams, TF-IDF ---------------------------------------------------------------------------------------
def _ng(b):
    """the n-gram orders of a batch: (min_n, max_n, sep)"""
    return {"E": (1, 2), "S": (2, 3), "S600": (1, 2), "SN": (1, 1), "M": (1, 3), "M5": (2, 2), "L": (1, 1)}[b.size] + (0x20,)


class Terms(Fam):
    """the four count calls and the two TF-IDF calls: CSR rows of one batch"""
    records, modes = ("indices", "data"), CAP_MODES

    def __init__(self, env, mode, entry, hashed, grams, tfidf=False):
        self.entry, self.hashed, self.grams, self.tfidf = entry, hashed, grams, tfidf
        if tfidf:
            self.modes = CAP_MODES + ("badcol",)
        super().__init__(env, mode)

    def opts(self, b):
        """(smooth_idf, sublinear_tf, norm) of a TF-IDF step: both smoothing modes, by the width of the occurrence"""
        return bool(self.odd), b.content == cs.SPARSE, NORMS[b.size]

    def full(self, b):
        r = self.env.ref(b)
        ng = _ng(b) if (self.grams or self.tfidf) else (1, 1, 0x20)
        if self.hashed:
            indptr, indices, data, total = r.hashed_csr(_hash, NC, True, *ng)
            w = {"indptr": indptr, "indices": indices, "data": data, "nnz": int(indptr[-1]), "total": total}
        else:
            indptr, indices, data, oov, total = r.vocab_csr(VOCAB, *ng)
            w = {"indptr": indptr, "oov": oov, "indices": indices, "data": data, "nnz": int(indptr[-1]), "total": total}
        if self.tfidf:
            smooth, sub, norm = self.opts(b)
            want = tfidf_ref.weigh(indptr, indices, data, tfidf_ref.idf(FROZEN_DF, FROZEN_DOCS, smooth), sub, norm)
            w["data"] = cs.Approx(want, tfidf_ref.bounds(indptr, norm))
            del w["total"]
        return w

    def run(self, b):
        env, lib, w = self.env, self.env.lib, self.cached(b)
        need = w["nnz"]
        indptr = self.out(b.n_str + 1, self.dt)
        oov = None if self.hashed else self.out(b.n_str, self.dt)
        indices, data = self.rec(need, np.int32), self.rec(need, np.float32 if self.tfidf else np.int32)
        nnz, total = C.c_int64(-1), C.c_int64(-1)
        ng = list(_ng(b)) if (self.grams or self.tfidf) else []
        head = [env.inp(b.u8), self.offs(b.boff), b.n_str, b.total_bytes]
        n_feat = NC + 1 if self.mode == "badcol" else NC
        vocab = (env.vocab_bad if self.mode == "badcol" else env.vocab).handle
        if self.tfidf:
            smooth, sub, norm = self.opts(b)
            opts = (1 if smooth else 0) | (2 if sub else 0) | NORM_BIT[norm]
            mid = [SEED, n_feat, 1] + ng if self.hashed else [vocab] + ng
            tail = [indptr.ptr] + ([] if self.hashed else [oov.ptr]) + [P(indices), P(data), self.cap(need), C.byref(nnz), self.flags, self.stream]
            rc = getattr(lib, self.entry)(*head, *mid, env.idf_frozen.handle, opts, *tail)
            scalars = {"nnz": nnz.value}
        else:
            mid = [SEED, NC, 1] + ng if self.hashed else [vocab] + ng
            tail = [indptr.ptr] + ([] if self.hashed else [oov.ptr]) + [P(indices), P(data), self.cap(need), C.byref(nnz), C.byref(total), self.flags,
                                                                         self.stream]
            rc = getattr(lib, self.entry)(*head, *mid, *tail)
            scalars = {"nnz": nnz.value, "total": total.value}
        outs = [("indptr", indptr, b.n_str + 1), ("oov", oov, b.n_str), ("indices", indices, need), ("data", data, need)]
        if self.mode == "badcol" and not self.hashed:
            # the vocabulary form is refused behind its kernels: host entry buffers stay untouched, device buffers hold the counts
            outs = [] if env.device else outs[2:]
        return rc, outs, scalars

    def expect(self, b):
        want = super().expect(b)
        if self.mode == "badcol" and not self.hashed:
            for k in ("indptr", "oov") + (("indices", "data") if self.env.device else ()):
                want.pop(k, None)
        return want


class IdfUpdateText(Fam):
    """latok_idf_update_utf8_bytes_batch into the accumulating idf, then latok_idf_read: even occurrences take the vocabulary with the
    batch's n-gram orders, odd ones the hashed unigrams"""
    entry, stateful_family, has_width = "latok_idf_update_utf8_bytes_batch", True, False
    modes = ("fit", "decreasing")

    def full(self, b):
        env, r = self.env, self.env.ref(b)
        k = (b.key, self.odd)
        if k not in self._full:
            if self.odd:
                indptr, indices = r.hashed_csr(_hash, NC, True)[:2]
            else:
                indptr, indices = r.vocab_csr(VOCAB, *_ng(b))[:2]
            self._full[k] = (tfidf_ref.document_frequency(indices, NC), int(indptr[-1]), r.n_tokens)      # (n_tokens_out: the TOKEN total)
        df, nnz, total = self._full[k]
        if self.mode == "fit":
            env.acc_df += df
            env.acc_docs += b.n_str
        return {"nnz": nnz, "total": total, "df": env.acc_df.copy(), "n_docs": np.array([env.acc_docs])}

    def run(self, b):
        env, nnz, total = self.env, C.c_int64(-1), C.c_int64(-1)
        ng = (1, 1, 0x20) if self.odd else _ng(b)
        rc = env.lib.latok_idf_update_utf8_bytes_batch(env.inp(b.u8), self.offs(b.boff), b.n_str, b.total_bytes, None if self.odd else env.vocab.handle,
                                                       SEED, NC if self.odd else 0, *ng, env.idf_acc.handle, C.byref(nnz), C.byref(total),
                                                       self.flags, self.stream)
        st = env.state()
        self.read = {"df": st["state: idf df"], "n_docs": st["state: idf n_docs"]}
        return rc, [], {"nnz": nnz.value, "total": total.value}

    def call(self, b, occ):
        res = super().call(b, occ)
        if self.mode == "fit":
            res.update(self.read)
        return res

    def expect(self, b):
        want = super().expect(b)
        if self.mode != "fit":
            for k in ("df", "n_docs"):
                want.pop(k, None)
        return want


# ---- WordPiece, fold, counter -------------------------------------------------------------------------------------------------------
class WordPieceIds(Fam):
    entry, records, modes = "latok_wordpiece_ids_utf8_bytes_batch", ("ids", "spans"), CAP_MODES

    def full(self, b):
        r = self.env.ref(b)
        indptr, ids, spans = wpr.cut_rows(b.u8, b.boff, r.counts, r.byte_spans.tolist(), WP_DICT, cs.WP_PREFIX, 100, WP_UNK)
        return {"indptr": np.array(indptr, np.int64), "ids": np.array(ids, np.int32), "spans": np.array(spans, np.int64).reshape(-1, 2),
                "n_pieces": len(ids), "n_tokens": r.n_tokens}

    def run(self, b):
        env, need = self.env, self.cached(b)["n_pieces"]
        indptr, ids, spans = self.out(b.n_str + 1, self.dt), self.rec(need, np.int32), self.rec(need, self.dt, (2,))
        n, n_tok = C.c_int64(-1), C.c_int64(-1)
        rc = env.lib.latok_wordpiece_ids_utf8_bytes_batch(env.inp(b.u8), self.offs(b.boff), b.n_str, b.total_bytes, env.wp.handle, WP_UNK, indptr.ptr,
                                                          P(ids), P(spans), self.cap(need), C.byref(n), C.byref(n_tok), self.flags, self.stream)
        return rc, [("indptr", indptr, b.n_str + 1), ("ids", ids, need), ("spans", spans, need)], {"n_pieces": n.value, "n_tokens": n_tok.value}


class WordPiecePadded(Fam):
    entry, has_width, modes = "latok_wordpiece_padded_utf8_bytes_batch", False, ("fit", "decreasing")

    def full(self, b):
        r = self.env.ref(b)
        indptr, ids, _ = wpr.cut_rows(b.u8, b.boff, r.counts, r.byte_spans.tolist(), WP_DICT, cs.WP_PREFIX, 100, WP_UNK)
        rows, lengths = np.full((b.n_str, WP_LEN), WP_PAD, np.int32), np.zeros(b.n_str, np.int32)
        for s in range(b.n_str):
            row = [WP_CLS] + ids[indptr[s]:indptr[s + 1]][:WP_LEN - 2] + [WP_SEP]
            rows[s, :len(row)], lengths[s] = row, len(row)
        return {"input_ids": rows, "lengths": lengths, "n_pieces": len(ids)}

    def run(self, b):
        env = self.env
        ids, lengths, n = self.out(b.n_str, np.int32, (WP_LEN,)), self.out(b.n_str, np.int32), C.c_int64(-1)
        rc = env.lib.latok_wordpiece_padded_utf8_bytes_batch(env.inp(b.u8), self.offs(b.boff), b.n_str, b.total_bytes, env.wp.handle, WP_UNK, WP_LEN, 1,
                                                             WP_CLS, WP_SEP, WP_PAD, ids.ptr, lengths.ptr, C.byref(n), self.flags, self.stream)
        return rc, [("input_ids", ids, b.n_str), ("lengths", lengths, b.n_str)], {"n_pieces": n.value}


class Fold(Fam):
    entry, has_width, records, modes = "latok_fold_utf8_bytes_batch", False, ("bytes",), CAP_MODES

    def bits(self):
        return fold_ref.UNCASED if self.odd else fold_ref.ALL

    def full(self, b):
        out, off = fold_ref.fold_batch(b.u8, b.boff, self.bits())
        return {"bytes": out, "out_off": off, "n": int(off[-1])}

    def run(self, b):
        env, need = self.env, self.cached(b)["n"]
        out, off, n = self.rec(need, np.uint8), self.out(b.n_str + 1, np.int64), C.c_int64(-1)
        rc = env.lib.latok_fold_utf8_bytes_batch(env.inp(b.u8), self.offs(b.boff), b.n_str, b.total_bytes, self.bits(), P(out), self.cap(need), off.ptr,
                                                 C.byref(n), self.flags, self.stream)
        return rc, [("bytes", out, need), ("out_off", off, b.n_str + 1)], {"n": n.value}


class Count(Fam):
    """latok_count_tokens_utf8_bytes_batch into the context's counter, then latok_counter_read: the words in byte order"""
    entry, stateful_family, has_width = "latok_count_tokens_utf8_bytes_batch", True, False
    modes = ("fit", "decreasing")

    @staticmethod
    def table(words):
        order = sorted(words)
        off = np.zeros(len(order) + 1, np.int64)
        np.cumsum([len(w) for w in order], out=off[1:])
        return {"words": np.frombuffer(b"".join(order), np.uint8), "word_off": off, "word_counts": np.array([words[w] for w in order], np.uint64)}

    def full(self, b):
        env, r = self.env, self.env.ref(b)
        if self.mode == "fit":
            for t in r.tokens:
                env.acc_words[t] = env.acc_words.get(t, 0) + 1
            env.acc_tokens += r.n_tokens
        w = {"stats4": np.array([r.n_tokens, r.n_tokens, 0, 0], np.int64)}
        w.update(self.table(env.acc_words))
        return w

    def run(self, b):
        env, lib = self.env, self.env.lib
        st = np.full(4, -1, np.int64)
        rc = lib.latok_count_tokens_utf8_bytes_batch(env.inp(b.u8), self.offs(b.boff), b.n_str, b.total_bytes, env.counter.handle, st.ctypes.data,
                                                     self.flags, self.stream)
        self.read = {}
        if self.mode == "fit":
            words, counts = env.counter.items()
            self.read = dict(self.table(dict(zip(words, (int(c) for c in counts)))), stats4=st)
        return rc, [], {}

    def call(self, b, occ):
        res = super().call(b, occ)
        res.update(self.read)
        return res

    def expect(self, b):
        want = super().expect(b)
        if self.mode != "fit":
            for k in ("stats4", "words", "word_off", "word_counts"):
                want.pop(k, None)
        return want


# ---- caller CSR ---------------------------------------------------------------------------------------------------------------------
class Csr(Fam):
    """latok_idf_update_csr (into the accumulating idf) / latok_tfidf_csr (under the frozen idf) on the batch's reference term counts"""
    modes = ("fit", "decreasing", "badcol")

    def __init__(self, env, mode, tfidf):
        self.tfidf, self.entry, self.stateful_family = tfidf, "latok_tfidf_csr" if tfidf else "latok_idf_update_csr", not tfidf
        self.records = ("data",) if tfidf else ()
        super().__init__(env, mode)

    def csr(self, b):
        k = ("csr", b.key)
        if k not in self._full:
            self._full[k] = self.env.ref(b).vocab_csr(VOCAB)[:3]
        return self._full[k]

    def opts(self, b):
        return bool(self.odd), b.content == cs.DENSE, NORMS[b.size]

    def full(self, b):
        env = self.env
        indptr, indices, data = self.csr(b)
        if self.tfidf:
            smooth, sub, norm = self.opts(b)
            want = tfidf_ref.weigh(indptr, indices, data, tfidf_ref.idf(FROZEN_DF, FROZEN_DOCS, smooth), sub, norm)
            return {"data": cs.Approx(want, tfidf_ref.bounds(indptr, norm))}
        if self.mode == "fit":
            env.acc_df += tfidf_ref.document_frequency(indices, NC)
            env.acc_docs += b.n_str
        return {"df": env.acc_df.copy(), "n_docs": np.array([env.acc_docs])}

    def run(self, b):
        env = self.env
        indptr, indices, data = self.csr(b)
        nnz = indices.size
        if self.mode == "badcol":
            indices = indices.copy()
            indices[nnz // 2] = NC
        ip = indptr.astype(self.dt)
        p_ip = self.offs(ip) if self.mode == "decreasing" else env.inp(ip, cache=False)
        p_ix = env.inp(indices, cache=False)
        self.read = {}
        if self.tfidf:
            smooth, sub, norm = self.opts(b)
            out = self.out(nnz, np.float32)
            rc = env.lib.latok_tfidf_csr(p_ip, p_ix, env.inp(data, cache=False), b.n_str, nnz, env.idf_frozen.handle,
                                         (1 if smooth else 0) | (2 if sub else 0) | NORM_BIT[norm], out.ptr, self.flags, self.stream)
            return rc, [("data", out, nnz)], {}
        rc = env.lib.latok_idf_update_csr(env.idf_acc.handle, p_ip, p_ix, b.n_str, nnz, self.flags, self.stream)
        if self.mode == "fit":
            st = env.state()
            self.read = {"df": st["state: idf df"], "n_docs": st["state: idf n_docs"]}
        return rc, [], {}

    def call(self, b, occ):
        res = super().call(b, occ)
        res.update(self.read)
        return res

    def expect(self, b):
        want = super().expect(b)
        if self.mode != "fit":
            for k in ("df", "n_docs"):
                want.pop(k, None)
        return want


# ---- the reference's three native functions -----------------------------------------------------------------------------------------
class Matrix(Fam):
    """latok_parse_matrix / latok_combine_matrix_rows / latok_block_mask on the first code points of the batch: they stage through the
    host staging area the widening calls use"""
    asynchronous, has_width = True, False

    def __init__(self, env, mode, entry):
        self.entry = entry
        super().__init__(env, mode)

    def parts(self, b):
        k = ("m", b.key)
        if k not in self._full:
            o = self.env.oracle
            cps = np.ascontiguousarray(b.cps[:MATRIX_CHARS])
            m = o.gen_parse_matrix(cps) if cps.size else np.zeros((0, 25), np.int8)
            mt = np.ascontiguousarray(m.T)
            a1 = o.combine_matrix_rows(mt, C_MASK) if cps.size else np.zeros(0, np.int8)
            self._full[k] = (cps, m, mt, np.ascontiguousarray(a1 != 0, np.int8), np.ascontiguousarray(mt[5] != 0, np.int8))
        return self._full[k]

    def full(self, b):
        o = self.env.oracle
        cps, m, mt, a1, a2 = self.parts(b)
        if self.entry == "latok_parse_matrix":
            return {"out": m}
        if cps.size == 0:
            return {"out": np.zeros(0, np.int8)}
        return {"out": o.combine_matrix_rows(mt, C_SPLIT) if self.entry == "latok_combine_matrix_rows" else o.gen_block_mask(a1, a2)}

    def run(self, b):
        env, lib = self.env, self.env.lib
        cps, m, mt, a1, a2 = self.parts(b)
        n = cps.size
        if self.entry == "latok_parse_matrix":
            o = self.out(n, np.int8, (25,))
            rc = lib.latok_parse_matrix(env.inp(cps), n, o.ptr, self.flags, self.stream)
        elif self.entry == "latok_combine_matrix_rows":
            o = self.out(n, np.int8)
            rc = lib.latok_combine_matrix_rows(env.inp(mt), 25, n, n, 1, env.inp(C_SPLIT), 2, C_SPLIT.shape[0], C_SPLIT.shape[1], o.ptr, self.flags,
                                               self.stream)
        else:
            o = self.out(n, np.int8)
            rc = lib.latok_block_mask(env.inp(a1), env.inp(a2), n, o.ptr, self.flags, self.stream)
        return rc, [("out", o, n)], {}


class Rules(Fam):
    """latok_set_rules / latok_reset_rules as a step of a plan: no output, the return code"""
    has_width = False

    def __init__(self, env, name):
        self.entry, self.rule_name = "latok_set_rules(%s)" % name if name else "latok_reset_rules", name
        super().__init__(env)

    def full(self, b):
        return {}

    def run(self, b):
        from latok_amd import batch
        env = self.env
        if self.rule_name is None:
            batch.reset_rules()
        else:
            batch.set_rules(*RULE_SETS[self.rule_name])
        rc = 0
        env.rules = self.rule_name
        return rc, [], {}


# ---- the 35 families ----------------------------------------------------------------------------------------------------------------
def _makers():
    """[(entry point, maker(env, mode))] in the order of the header"""
    def compact(entry, form, what, uses_l):
        return entry, lambda env, mode="fit": Compact(env, mode, entry, form, what, uses_l)

    def mask(entry, form, attr, dtype, uses_l):
        return entry, lambda env, mode="fit": Mask(env, mode, entry, form, attr, dtype, uses_l)

    def terms(entry, hashed, grams, tfidf=False):
        return entry, lambda env, mode="fit": Terms(env, mode, entry, hashed, grams, tfidf)

    def plain(cls, *a):
        return (cls.entry if cls.entry else a[-1]), lambda env, mode="fit": cls(env, mode, *a)

    return [
        mask("latok_split_mask_batch", "cps", "cp_mask", np.uint64, True),
        mask("latok_split_values_batch", "cps", "values", np.uint8, True),
        compact("latok_split_offsets_batch", "cps", "offsets", True),
        compact("latok_token_spans_batch", "cps", "spans", True),
        compact("latok_token_features_batch", "cps", "features", True),
        compact("latok_token_features_kind_batch", "k1", "features", True),
        compact("latok_token_spans_kind_batch", "k2", "spans", True),
        plain(Decode),
        plain(MaskUtf8),
        compact("latok_split_offsets_utf8_batch", "u8", "offsets", True),
        compact("latok_token_spans_utf8_batch", "u8", "spans", True),
        compact("latok_token_features_utf8_batch", "u8", "features", True),
        mask("latok_split_mask_utf8_bytes_batch", "bytes", "byte_mask", np.uint64, False),
        compact("latok_split_offsets_utf8_bytes_batch", "bytes", "offsets", False),
        compact("latok_token_spans_utf8_bytes_batch", "bytes", "spans", False),
        compact("latok_token_features_utf8_bytes_batch", "bytes", "features", False),
        plain(Join),
        ("latok_token_hashes_utf8_bytes_batch", lambda env, mode="fit": HashesIds(env, mode, False)),
        ("latok_token_ids_utf8_bytes_batch", lambda env, mode="fit": HashesIds(env, mode, True)),
        terms("latok_term_counts_utf8_bytes_batch", False, False),
        terms("latok_hashed_term_counts_utf8_bytes_batch", True, False),
        terms("latok_ngram_counts_utf8_bytes_batch", False, True),
        terms("latok_hashed_ngram_counts_utf8_bytes_batch", True, True),
        terms("latok_tfidf_utf8_bytes_batch", False, True, True),
        terms("latok_hashed_tfidf_utf8_bytes_batch", True, True, True),
        plain(IdfUpdateText),
        plain(WordPieceIds),
        plain(WordPiecePadded),
        plain(Fold),
        plain(Count),
        ("latok_idf_update_csr", lambda env, mode="fit": Csr(env, mode, False)),
        ("latok_tfidf_csr", lambda env, mode="fit": Csr(env, mode, True)),
        ("latok_parse_matrix", lambda env, mode="fit": Matrix(env, mode, "latok_parse_matrix")),
        ("latok_combine_matrix_rows", lambda env, mode="fit": Matrix(env, mode, "latok_combine_matrix_rows")),
        ("latok_block_mask", lambda env, mode="fit": Matrix(env, mode, "latok_block_mask")),
    ]


def _families(env):
    fams = [make(env) for _, make in _makers()]
    assert len(fams) == 35 and len({f.name for f in fams}) == 35
    return fams


def _refusers(env, makers=None):
    """every refusing step of the issue that the pointer mode allows"""
    out = []
    for _, make in (_makers() if makers is None else makers):
        for mode in make(env).modes[1:]:
            if mode == "decreasing" and env.device:
                continue                               # device-resident row offsets are the caller's promise
            out.append(make(env, mode))
    return out


# ---- the ten later families: word lists, built without the library --------------------------------------------------------------------
PIECE_MAX_BYTES, PIECE_LEN, BPE_MERGES = 24, 12, 60             # LONG_WORDS run to 29 bytes: a SPARSE batch holds over-long tokens
BPE_UNK, BPE_BOS, BPE_EOS, BPE_PAD = -3, 1001, 1002, 1003       # none of them is an id of the decoder over BPE_WORDS
UNI_UNK, UNI_BOS, UNI_EOS, UNI_PAD, UNI_UNK_SCORE = -5, 2001, 2002, 2003, -20.0
DETOK_WP_UNK = -9                                               # the unknown piece of the WordPiece rows: not an id of the decoder
_LONG = [w.encode() for w in cs.LONG_WORDS]
# BPE: every single byte but `q` and 0xF0 (a SPARSE word with a q and the 4-byte letter of a DENSE batch leave unk pieces), the merges of
# the long words, then what a DENSE batch merges: the 2- and 3-byte letters and " a" .. " e" (lead_space puts the space in front)
BPE_TRAINED = bpe_ref.train(_LONG, BPE_MERGES, base=[x for x in range(256) if x not in (ord("q"), 0xF0)])
BPE_WORDS = BPE_TRAINED + [w for w in [x.encode("utf-8") for x in cs.WIDE_LETTERS[:4]] + [b" " + c.encode() for c in "abcde"] if w not in BPE_TRAINED]
GPT2_WORDS = BPE_WORDS + [b" " + w for w in BPE_WORDS if len(w) > 1 and not w.startswith(b" ")] + [b" ", b"  ", b"\t"]
BPE_DICT, GPT2_DICT = bpe_ref.rank_dict(BPE_WORDS), bpe_ref.rank_dict(GPT2_WORDS)
assert len(GPT2_WORDS) < BPE_BOS and len(BPE_TRAINED) == 254 + BPE_MERGES and len(set(BPE_WORDS)) == len(BPE_WORDS)      # (ranks are positions)


def _uni_words():
    """single letters but q and x, the wide letters, the 2 .. 6-byte prefixes of the long words; every third also behind the marker; the
    marker itself"""
    plain = [c.encode() for c in cs.ASCII_LETTERS if c not in "qx"] + [w.encode("utf-8") for w in cs.WIDE_LETTERS] + \
        sorted({w[:k] for w in _LONG for k in range(2, 7)})
    words = []
    for i, w in enumerate(plain):
        words.append(w)
        if i % 3 == 0:
            words.append(unigram_ref.MARKER + w)
    return words + [unigram_ref.MARKER]


UNI_WORDS = _uni_words()
UNI_SCORES = np.array([-(8 + (i * 5) % 11) / 8 for i in range(len(UNI_WORDS))], np.float32)       # multiples of 1/8: every sum is exact
UNI_DICT = unigram_ref.word_dict(UNI_WORDS)


def _cg_words():
    """cs.VOCAB_WORDS, then character grams of the long words and of the one-letter tokens, pads included"""
    extra = [g for w in _LONG[::4] for g in [x[2] for x in chargram_ref.token_grams(w, 2, 3)][::3]]
    extra += [b" " + c.encode() for c in cs.ASCII_LETTERS[:12]] + [c.encode() + b" " for c in cs.ASCII_LETTERS[:6]] + [b" a ", b" b ", b" "]
    out, seen = list(cs.VOCAB_WORDS), set(cs.VOCAB_WORDS)
    for g in extra:
        if g not in seen:
            seen.add(g)
            out.append(g)
    return out


CG_WORDS = _cg_words()
CG_VOCAB = {w: i for i, w in reversed(list(enumerate(CG_WORDS)))}
DETOK_BPE_MAP, DETOK_WP_MAP = detok_ref.id_map(BPE_WORDS), detok_ref.id_map(cs.WP_WORDS)
DETOK_BPE_SKIP = (BPE_DICT[b"a"], BPE_DICT[b"e"])               # two ids that occur in the rows
DETOK_WP_SKIP = (WP_DICT[b"a"], WP_DICT[b"##e"])


# ---- their references: one cut of a batch, kept with the batch ------------------------------------------------------------------------
def _pretok(b):
    """(counts, spans) of GPT-2's pre-tokens of every string; no rule table has a say"""
    k = ("pretok", None, None)
    if k not in b._ref:
        raw, counts, spans = b.u8.tobytes(), [], []
        for s in range(b.n_str):
            p = pretok_ref.pretokens(raw[int(b.boff[s]):int(b.boff[s + 1])])
            counts.append(len(p))
            spans += p
        b._ref[k] = (np.array(counts, np.int64), np.array(spans, np.int64).reshape(-1, 2))
    return b._ref[k]


@functools.lru_cache(maxsize=None)
def _bpe_cut(token, gpt2):
    return tuple(bpe_ref.cut(token, GPT2_DICT if gpt2 else BPE_DICT, PIECE_MAX_BYTES, BPE_UNK))


@functools.lru_cache(maxsize=None)
def _uni_cut(token, marked):
    return tuple(unigram_ref.cut(token, marked, UNI_DICT, UNI_SCORES, UNI_UNK_SCORE, unigram_ref.MARKER, True, PIECE_MAX_BYTES, UNI_UNK))


@functools.lru_cache(maxsize=None)
def _wp_cut(token):
    return tuple(wpr.cut(token, WP_DICT, cs.WP_PREFIX, 100, DETOK_WP_UNK))


def _cut_rows(b, counts, spans, kind):
    """bpe_ref.cut_rows / unigram_ref.cut_rows / wordpiece_ref.cut_rows with every distinct token cut once (a batch repeats few tokens
    many times); tests/test_call_sequences_host.py holds this loop to the three helpers, in its four kinds"""
    raw, indptr, ids, out, k = b.u8.tobytes(), [0], [], [], 0
    for s in range(b.n_str):
        base, prev = int(b.boff[s]), None
        for _ in range(int(counts[s])):
            a, e = spans[k]
            k += 1
            if kind == "uni":
                pieces = _uni_cut(raw[base + a:base + e], unigram_ref.is_marked(prev, a))
            elif kind == "wp":
                pieces = _wp_cut(raw[base + a:base + e])
            else:
                if kind == "bpe" and a > 0 and raw[base + a - 1] == 0x20:       # lead_space
                    a -= 1
                pieces = _bpe_cut(raw[base + a:base + e], kind == "gpt2")
            for pid, p0, p1 in pieces:
                ids.append(pid)
                out.append((a + p0, a + p1))
            prev = e
        indptr.append(len(ids))
    return indptr, ids, out


def _pieces(env, b, kind, rules=True):
    """(indptr int64, ids int32, spans int64 [n, 2], n_tokens) of one cut of a batch.  kind: "bpe" (latok's tokens, the space in front),
    "gpt2" (GPT-2's pre-tokens), "uni", "wp" (the WordPiece rows the decoder gets, unknown = DETOK_WP_UNK).  rules=False: the tokens
    under the built-in rules whatever the context holds"""
    k = ("pieces", kind, env.rules if (rules and kind != "gpt2") else None)
    if k not in b._ref:
        if kind == "gpt2":
            counts, spans = _pretok(b)
            cut, n_tok = _cut_rows(b, counts, spans.tolist(), kind), len(spans)
        else:
            r = env.ref(b) if rules else cs.reference(env.oracle, b)
            n_tok = r.n_tokens
            cut = _cut_rows(b, r.counts, r.byte_spans.tolist(), kind)
        b._ref[k] = (np.array(cut[0], np.int64), np.array(cut[1], np.int32).reshape(-1), np.array(cut[2], np.int64).reshape(-1, 2), n_tok)
    return b._ref[k]


def _padded(indptr, ids, n_str, bos, eos, pad):
    """the [n_str, PIECE_LEN] block with its specials, and the lengths: row s = bos, the first PIECE_LEN - 2 ids of row s, eos, then pad"""
    take = np.minimum(np.diff(indptr), PIECE_LEN - 2)
    rows = np.full((n_str, PIECE_LEN), pad, np.int32)
    rows[:, 0] = bos
    cols = np.arange(PIECE_LEN - 2)
    held = cols[None, :] < take[:, None]
    rows[:, 1:PIECE_LEN - 1][held] = ids[(indptr[:-1, None] + cols[None, :])[held]]
    rows[np.arange(n_str), take + 1] = eos
    return rows, (take + 2).astype(np.int32)


def _decoded(texts, unknown):
    off = np.zeros(len(texts) + 1, np.int64)
    np.cumsum([len(t) for t in texts], out=off[1:])
    return {"bytes": np.frombuffer(b"".join(texts), np.uint8), "out_off": off, "n": int(off[-1]), "n_unknown": unknown}


# ---- the ten families -----------------------------------------------------------------------------------------------------------------
class Later(Fam):
    """a later family: what full() gives is a function of (family, batch, width, rules) alone and is kept with the batch, for every test
    of the session"""

    def cached(self, b):
        k = ("full", self.entry, self.odd, self.env.rules)
        if k not in b._ref:
            b._ref[k] = self.full(b)
        return b._ref[k]


@functools.lru_cache(maxsize=None)
def _token_grams(token, lo, hi, pad):
    return tuple(chargram_ref.row_grams((token,), lo, hi, pad))


class CharGrams(Later):
    """latok_chargram_counts_utf8_bytes_batch / latok_hashed_chargram_counts_utf8_bytes_batch: orders 2 .. 3 on even occurrences, 1 .. 4 on
    odd ones; the hashed form alternates its sign on the odd ones"""
    boundary = True
    records, modes = ("indices", "data"), CAP_MODES
    PAD = 0x20

    def __init__(self, env, mode, entry, hashed):
        self.entry, self.hashed = entry, hashed
        super().__init__(env, mode)

    def orders(self):
        return (1, 4) if self.odd else (2, 3)

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def key(gram):
        h = _hash(gram)
        h = h - (1 << 32) if h >= (1 << 31) else h
        return abs(h) % NC, (-1 if h < 0 else 1)

    def full(self, b):
        k = ("chargrams", self.orders(), self.env.rules)                                    # the two forms share the grams
        if k not in b._ref:
            b._ref[k] = [[g for t in row for g in _token_grams(t, *self.orders(), self.PAD)] for row in self.env.ref(b).rows()]
        grams = b._ref[k]
        total = sum(len(g) for g in grams)
        if self.hashed:
            indptr, indices, data = cs._csr([[(self.key(x)[0], self.key(x)[1] if self.odd else 1) for x in g] for g in grams])
            return {"indptr": indptr, "indices": indices, "data": data, "nnz": int(indptr[-1]), "total": total}
        rows = [[(CG_VOCAB[x], 1) for x in g if x in CG_VOCAB] for g in grams]
        indptr, indices, data = cs._csr(rows)
        oov = np.array([len(g) - len(r) for g, r in zip(grams, rows)], np.int64)
        return {"indptr": indptr, "oov": oov, "indices": indices, "data": data, "nnz": int(indptr[-1]), "total": total}

    def run(self, b):
        env, need = self.env, self.cached(b)["nnz"]
        indptr, oov = self.out(b.n_str + 1, self.dt), None if self.hashed else self.out(b.n_str, self.dt)
        indices, data = self.rec(need, np.int32), self.rec(need, np.int32)
        nnz, total = C.c_int64(-1), C.c_int64(-1)
        mid = [SEED, NC, self.odd] if self.hashed else [env.cg_vocab.handle]
        tail = [indptr.ptr] + ([] if self.hashed else [oov.ptr]) + [P(indices), P(data), self.cap(need), C.byref(nnz), C.byref(total), self.flags, self.stream]
        rc = getattr(env.lib, self.entry)(env.inp(b.u8), self.offs(b.boff), b.n_str, b.total_bytes, *mid, *self.orders(), self.PAD, *tail)
        outs = [("indptr", indptr, b.n_str + 1), ("oov", oov, b.n_str), ("indices", indices, need), ("data", data, need)]
        return rc, outs, {"nnz": nnz.value, "total": total.value}


class PieceIds(Later):
    """latok_bpe_ids_utf8_bytes_batch (on latok's tokens; on GPT-2's pre-tokens) / latok_unigram_ids_utf8_bytes_batch"""
    records, modes = ("ids", "spans"), CAP_MODES

    def __init__(self, env, mode, entry, fn, kind, obj, unk):
        self.entry, self.fn, self.kind, self.obj, self.unk, self.boundary = entry, fn, kind, obj, unk, kind != "gpt2"
        super().__init__(env, mode)

    def full(self, b):
        indptr, ids, spans, n_tok = _pieces(self.env, b, self.kind)
        return {"indptr": indptr, "ids": ids, "spans": spans, "n_pieces": int(ids.size), "n_tokens": n_tok}

    def run(self, b):
        env, need = self.env, self.cached(b)["n_pieces"]
        indptr, ids, spans = self.out(b.n_str + 1, self.dt), self.rec(need, np.int32), self.rec(need, self.dt, (2,))
        n, n_tok = C.c_int64(-1), C.c_int64(-1)
        rc = getattr(env.lib, self.fn)(env.inp(b.u8), self.offs(b.boff), b.n_str, b.total_bytes, getattr(env, self.obj).handle, self.unk, indptr.ptr,
                                       P(ids), P(spans), self.cap(need), C.byref(n), C.byref(n_tok), self.flags, self.stream)
        return rc, [("indptr", indptr, b.n_str + 1), ("ids", ids, need), ("spans", spans, need)], {"n_pieces": n.value, "n_tokens": n_tok.value}


class PiecePadded(Later):
    """latok_bpe_padded_utf8_bytes_batch (the latok-token object on even occurrences, the GPT-2 object on odd ones) /
    latok_unigram_padded_utf8_bytes_batch: PIECE_LEN cells a row, specials on"""
    has_width, boundary, modes = False, True, ("fit", "decreasing")

    def __init__(self, env, mode, entry, kinds, objs, ids4):
        self.entry, self.kinds, self.objs, self.ids4 = entry, kinds, objs, ids4           # ids4: (unk, bos, eos, pad)
        super().__init__(env, mode)

    def full(self, b):
        indptr, ids, _, _ = _pieces(self.env, b, self.kinds[self.odd])
        rows, lengths = _padded(indptr, ids, b.n_str, *self.ids4[1:])
        return {"input_ids": rows, "lengths": lengths, "n_pieces": int(ids.size)}

    def run(self, b):
        env = self.env
        unk, bos, eos, pad = self.ids4
        ids, lengths, n = self.out(b.n_str, np.int32, (PIECE_LEN,)), self.out(b.n_str, np.int32), C.c_int64(-1)
        rc = getattr(env.lib, self.entry)(env.inp(b.u8), self.offs(b.boff), b.n_str, b.total_bytes, getattr(env, self.objs[self.odd]).handle, unk,
                                          PIECE_LEN, 1, bos, eos, pad, ids.ptr, lengths.ptr, C.byref(n), self.flags, self.stream)
        return rc, [("input_ids", ids, b.n_str), ("lengths", lengths, b.n_str)], {"n_pieces": n.value}


class Pretokens(Later):
    """latok_pretokens_utf8_bytes_batch with LATOK_PRETOK_GPT2: the other front, on its own"""
    entry, records, modes = "latok_pretokens_utf8_bytes_batch", ("items",), CAP_MODES
    GPT2 = 1

    def full(self, b):
        counts, spans = _pretok(b)
        return {"counts": counts, "items": spans, "n": int(spans.shape[0])}

    def run(self, b):
        env, need = self.env, self.cached(b)["n"]
        counts, items, n = self.out(b.n_str, self.dt), self.rec(need, self.dt, (2,)), C.c_int64(-1)
        rc = env.lib.latok_pretokens_utf8_bytes_batch(env.inp(b.u8), self.offs(b.boff), b.n_str, b.total_bytes, self.GPT2, counts.ptr, P(items),
                                                      self.cap(need), C.byref(n), self.flags, self.stream)
        return rc, [("counts", counts, b.n_str), ("items", items, need)], {"n": n.value}


class DetokCsr(Later):
    """latok_detok_csr: on even occurrences the CONCAT decoder over BPE_WORDS on the batch's reference BPE ids (int64 indptr), on odd ones
    the WORDPIECE decoder over cs.WP_WORDS on its reference WordPiece ids (int32 indptr).  The unknown pieces of either cut carry an id
    the decoder does not hold; two ids that occur are skipped.  The rows are those under the built-in rules: no rule table has a say"""
    entry, records, modes = "latok_detok_csr", ("bytes",), CAP_MODES

    def parts(self):
        return ("wp", "detok_wp", DETOK_WP_MAP, detok_ref.WORDPIECE, DETOK_WP_SKIP) if self.odd else \
               ("bpe", "detok_bpe", DETOK_BPE_MAP, detok_ref.CONCAT, DETOK_BPE_SKIP)

    def full(self, b):
        kind, _, d, mode, skip = self.parts()
        indptr, ids, _, _ = _pieces(self.env, b, kind, rules=False)
        ids, at = ids.tolist(), indptr.tolist()
        rows = [ids[at[s]:at[s + 1]] for s in range(b.n_str)]
        return _decoded(*detok_ref.decode(rows, d, mode, cs.WP_PREFIX, b" ", skip))

    def run(self, b):
        env, need = self.env, self.cached(b)["n"]
        kind, obj, _, _, skip = self.parts()
        indptr, ids, _, _ = _pieces(env, b, kind, rules=False)
        ip = indptr.astype(self.dt)
        p_ip = self.offs(ip) if self.mode == "decreasing" else env.inp(ip, cache=False)
        skip = np.array(skip, np.int32)                                                    # a host pointer in every mode
        out, off, n, unk = self.rec(need, np.uint8), self.out(b.n_str + 1, np.int64), C.c_int64(-1), C.c_int64(-1)
        rc = env.lib.latok_detok_csr(getattr(env, obj).handle, p_ip, env.inp(ids, cache=False), b.n_str, ids.size, skip.ctypes.data, skip.size, P(out),
                                     self.cap(need), off.ptr, C.byref(n), C.byref(unk), self.flags, self.stream)
        return rc, [("bytes", out, need), ("out_off", off, b.n_str + 1)], {"n": n.value, "n_unknown": unk.value}


class DetokPadded(Later):
    """latok_detok_padded on the reference padded BPE block: with its lengths on even occurrences (BOS and one id that occurs skipped, so
    that every EOS is an unknown id), with lengths = NULL and the pad id among the skipped ones on odd occurrences"""
    entry, has_width, records, modes = "latok_detok_padded", False, ("bytes",), ("fit", "short", "query")

    def block(self, b):
        k = ("block", None, None)
        if k not in b._ref:
            indptr, ids, _, _ = _pieces(self.env, b, "bpe", rules=False)
            b._ref[k] = _padded(indptr, ids, b.n_str, BPE_BOS, BPE_EOS, BPE_PAD)
        return b._ref[k]

    def skip(self):
        return (BPE_BOS, BPE_EOS, BPE_PAD) if self.odd else (BPE_BOS, DETOK_BPE_SKIP[0])

    def full(self, b):
        rows, lengths = self.block(b)
        return _decoded(*detok_ref.decode(detok_ref.padded_rows(rows.tolist(), None if self.odd else lengths.tolist()), DETOK_BPE_MAP, detok_ref.CONCAT,
                                          skip=self.skip()))

    def run(self, b):
        env, need = self.env, self.cached(b)["n"]
        rows, lengths = self.block(b)
        skip = np.array(self.skip(), np.int32)
        out, off, n, unk = self.rec(need, np.uint8), self.out(b.n_str + 1, np.int64), C.c_int64(-1), C.c_int64(-1)
        rc = env.lib.latok_detok_padded(env.detok_bpe.handle, env.inp(rows, cache=False), None if self.odd else env.inp(lengths, cache=False), b.n_str,
                                        PIECE_LEN, skip.ctypes.data, skip.size, P(out), self.cap(need), off.ptr, C.byref(n), C.byref(unk), self.flags,
                                        self.stream)
        return rc, [("bytes", out, need), ("out_off", off, b.n_str + 1)], {"n": n.value, "n_unknown": unk.value}


def _new_makers():
    """[(family name, maker(env, mode))] of the ten families that came after the 35, in the order of the header"""
    bpe, uni = "latok_bpe_ids_utf8_bytes_batch", "latok_unigram_ids_utf8_bytes_batch"

    def grams(entry, hashed):
        return entry, lambda env, mode="fit": CharGrams(env, mode, entry, hashed)

    def ids(entry, fn, kind, obj, unk):
        return entry, lambda env, mode="fit": PieceIds(env, mode, entry, fn, kind, obj, unk)

    def padded(entry, kinds, objs, ids4):
        return entry, lambda env, mode="fit": PiecePadded(env, mode, entry, kinds, objs, ids4)

    return [
        grams("latok_chargram_counts_utf8_bytes_batch", False),
        grams("latok_hashed_chargram_counts_utf8_bytes_batch", True),
        ids(bpe, bpe, "bpe", "bpe", BPE_UNK),
        ids(bpe + "[gpt2]", bpe, "gpt2", "bpe_gpt2", BPE_UNK),
        padded("latok_bpe_padded_utf8_bytes_batch", ("bpe", "gpt2"), ("bpe", "bpe_gpt2"), (BPE_UNK, BPE_BOS, BPE_EOS, BPE_PAD)),
        (Pretokens.entry, lambda env, mode="fit": Pretokens(env, mode)),
        ids(uni, uni, "uni", "uni", UNI_UNK),
        padded("latok_unigram_padded_utf8_bytes_batch", ("uni", "uni"), ("uni", "uni"), (UNI_UNK, UNI_BOS, UNI_EOS, UNI_PAD)),
        (DetokCsr.entry, lambda env, mode="fit": DetokCsr(env, mode)),
        (DetokPadded.entry, lambda env, mode="fit": DetokPadded(env, mode)),
    ]


N_OLD, N_NEW = 35, 10


def _all_families(env):
    """the 35, then the ten"""
    fams = _families(env) + [make(env) for _, make in _new_makers()]
    assert len(fams) == N_OLD + N_NEW and len({f.name for f in fams}) == N_OLD + N_NEW
    return fams


class _Session:
    """a fresh context with its objects, closed on the way out"""

    def __init__(self, gpu, oracle, pointers):
        from latok_amd import _lib
        self.args, self._lib = (gpu, oracle, pointers == "device"), _lib

    def __enter__(self):
        self.ctx = self._lib.Context(self._lib.default_device())
        self.ctx.__enter__()
        try:
            self.env = Env(*self.args)
            if self.env.device:
                self.env.upload_all(_batches())
        except BaseException:
            self.ctx.__exit__(None, None, None)
            self.ctx.destroy()
            raise
        return self.env

    def __exit__(self, *exc):
        try:
            self.env.lib.latok_reset_rules()
            self._lib.check(self.env.lib.latok_sync())
            self.env.close()
        finally:
            self.ctx.__exit__(None, None, None)
            self.ctx.destroy()
        return False


POINTERS = pytest.mark.parametrize("pointers", ["host", "device"])


def _pair_plan(fams):
    plan = cs.pair_cover(len(fams))
    keys = cs.rotation(plan, [f.uses_l for f in fams])
    return plan, [_batches()[k] for k in keys]


@POINTERS
def test_every_family_after_every_other(gpu, oracle, pointers):
    with _Session(gpu, oracle, pointers) as env:
        fams = _families(env)
        plan, sizes = _pair_plan(fams)
        assert len(plan) == 35 * 35 + 1 and len(set(cs.pairs_of(plan))) == 35 * 35
        assert cs.run(plan, fams, sizes) == 35 * 35 + 1


@POINTERS
def test_every_family_after_every_refusal(gpu, oracle, pointers):
    with _Session(gpu, oracle, pointers) as env:
        fams, refs = _families(env), _refusers(env)
        every = refs + fams
        plan = cs.after_each(range(len(refs)), range(len(refs), len(every)))
        assert len(plan) == 2 * len(refs) * 35 and len(refs) >= (50 if env.device else 80)
        B = _batches()
        follow = [("S", cs.SPARSE), ("M5", cs.SPARSE), ("E", cs.SPARSE), ("S600", cs.SPARSE), ("M", cs.SPARSE), ("S", cs.DENSE), ("M", cs.DENSE)]
        sizes = []
        for k in range(0, len(plan), 2):               # the refused batch is dense: on the single-wave route (S600 breaks it) and on two tiles
            refused = "M" if (k // 2) % 2 else "S600" if every[plan[k]].mode == "decreasing" else "S"
            sizes += [B[(refused, cs.DENSE)], B[follow[(k // 2) % len(follow)]]]
        assert cs.run(plan, every, sizes) == len(plan)


@POINTERS
def test_rules_do_not_leak_between_families(gpu, oracle, pointers):
    """every boundary family straight after latok_set_rules(all_columns) and straight after latok_reset_rules, a family that reads no rule
    (fold, tfidf_csr) between each pair"""
    with _Session(gpu, oracle, pointers) as env:
        fams = _families(env)
        fold = next(i for i, f in enumerate(fams) if f.entry == "latok_fold_utf8_bytes_batch")
        csr = next(i for i, f in enumerate(fams) if f.entry == "latok_tfidf_csr")
        every = fams + [Rules(env, "all_columns"), Rules(env, None)]
        on, off = len(fams), len(fams) + 1
        plan, n_boundary = [], 0
        for i, f in enumerate(fams):
            if f.boundary:
                plan += [on, i, fold if n_boundary % 2 else csr, off, i, csr if n_boundary % 2 else fold]
                n_boundary += 1
        assert n_boundary == 15
        B = _batches()
        shapes = [("M5", cs.DENSE), ("M", cs.SPARSE), ("S", cs.DENSE), ("S600", cs.SPARSE)]
        sizes = [B[shapes[(k // 3) % len(shapes)]] for k in range(len(plan))]
        assert cs.run(plan, every, sizes) == len(plan) == 6 * 15


def test_every_family_on_rotating_caller_streams(gpu, oracle):
    """device pointers, the pair plan, step k on stream k % 3 of {NULL, s1, s2}; the asynchronous calls (mask, values, the three native
    functions) are read only after the next step has been enqueued: that step waits for them on the device and shares their workspace"""
    with _Session(gpu, oracle, "device") as env:
        hip = env.lib              # the HIP runtime the library is linked against, looked up through its handle
        s1, s2 = C.c_void_p(), C.c_void_p()
        assert hip.hipStreamCreate(C.byref(s1)) == 0 and hip.hipStreamCreate(C.byref(s2)) == 0
        try:
            env.streams, env.defer, env.keep = [None, s1, s2], True, True
            fams = _families(env)
            plan, sizes = _pair_plan(fams)
            used = set()
            assert cs.run(plan, fams, sizes, on_step=lambda k, f, b, o: used.add((f.name, (k % 3)))) == 35 * 35 + 1
            assert used == {(fams[f].name, k % 3) for k, f in enumerate(plan)} and len(used) >= 3 * 35 - 3
            assert hip.hipStreamSynchronize(s1) == 0 and hip.hipStreamSynchronize(s2) == 0
            env._lib.check(env.lib.latok_sync())
        finally:
            env.streams = None
            hip.hipStreamDestroy(s1)
            hip.hipStreamDestroy(s2)


@POINTERS
def test_scan_epoch_wrap_inside_multi_scan_calls(gpu, oracle, pointers):
    """the 18-bit scan epoch wraps between two scans of one call: each multi-scan family starts four epochs in front of the wrap at M5,
    then one full turn of all families"""
    multi = ("latok_term_counts_utf8_bytes_batch", "latok_ngram_counts_utf8_bytes_batch", "latok_wordpiece_ids_utf8_bytes_batch",
             "latok_wordpiece_padded_utf8_bytes_batch", "latok_fold_utf8_bytes_batch", "latok_token_features_utf8_batch")
    with _Session(gpu, oracle, pointers) as env:
        fams = _families(env)
        B = _batches()
        gpu.latok_debug_set_scan_epoch.restype, gpu.latok_debug_set_scan_epoch.argtypes = C.c_int, [C.c_uint]
        for start in (0x3FFFE, 0x3FFFF, 0x3FFFD, 0x3FFFC):
            for name in multi:
                i = next(i for i, f in enumerate(fams) if f.entry == name)
                assert gpu.latok_debug_set_scan_epoch(start) == 0
                assert cs.run([i, i], fams, [B[("M5", cs.DENSE)], B[("M5", cs.SPARSE)]]) == 2
        assert gpu.latok_debug_set_scan_epoch(0x3FFFC) == 0
        turn = list(range(35))
        keys = cs.rotation(turn, [f.uses_l for f in fams])
        assert cs.run(turn, fams, [B[k] for k in keys]) == 35


# ---- the ten later families beside the 35 ---------------------------------------------------------------------------------------------
NEW = range(N_OLD, N_OLD + N_NEW)
# the later families that enqueue more than one device-wide scan per call (latok_amd/csrc/api.cpp): the char-gram calls (token rows, grams
# per token, the CSR tail) and the piece calls of BPE and Unigram (token rows, pieces per token), each behind the scan of the token front;
# the pre-tokens and the decoders scan once
NEW_MULTI_SCAN = ("latok_chargram_counts_utf8_bytes_batch", "latok_hashed_chargram_counts_utf8_bytes_batch", "latok_bpe_ids_utf8_bytes_batch",
                  "latok_bpe_ids_utf8_bytes_batch[gpt2]", "latok_bpe_padded_utf8_bytes_batch", "latok_unigram_ids_utf8_bytes_batch",
                  "latok_unigram_padded_utf8_bytes_batch")
RULE_FREE_NEW = ("latok_pretokens_utf8_bytes_batch", "latok_bpe_ids_utf8_bytes_batch[gpt2]", "latok_detok_csr")


def _touching_plan(fams):
    plan = cs.pair_cover_touching(len(fams), NEW)
    keys = cs.rotation(plan, [f.uses_l for f in fams])
    return plan, [_batches()[k] for k in keys]


def _touching_pairs():
    n = N_OLD + N_NEW
    return {(a, b) for a in range(n) for b in range(n) if a >= N_OLD or b >= N_OLD}


def _refusal_sizes(plan, every):
    """the batches of an after_each plan, as test_every_family_after_every_refusal picks them"""
    B = _batches()
    follow = [("S", cs.SPARSE), ("M5", cs.SPARSE), ("E", cs.SPARSE), ("S600", cs.SPARSE), ("M", cs.SPARSE), ("S", cs.DENSE), ("M", cs.DENSE)]
    sizes = []
    for k in range(0, len(plan), 2):
        refused = "M" if (k // 2) % 2 else "S600" if every[plan[k]].mode == "decreasing" else "S"
        sizes += [B[(refused, cs.DENSE)], B[follow[(k // 2) % len(follow)]]]
    return sizes


@POINTERS
def test_every_new_family_beside_every_family(gpu, oracle, pointers):
    """every ordered pair of the 45 families that has one of the ten later ones in it, each once: 45 * 45 - 35 * 35 = 800 pairs"""
    with _Session(gpu, oracle, pointers) as env:
        fams = _all_families(env)
        plan, sizes = _touching_plan(fams)
        pairs = cs.pairs_of(plan)
        assert len(plan) == 801 and len(pairs) == len(set(pairs)) == 800 and set(pairs) == _touching_pairs()
        assert cs.run(plan, fams, sizes) == 801


@POINTERS
def test_every_family_after_every_new_refusal_and_back(gpu, oracle, pointers):
    """every refusing mode of the ten later families in front of all 45, and every refusing mode of the 35 in front of the ten"""
    with _Session(gpu, oracle, pointers) as env:
        fams = _all_families(env)
        refs_new, refs_old = _refusers(env, _new_makers()), _refusers(env)
        every = refs_new + refs_old + fams
        first = len(refs_new) + len(refs_old)
        plan = cs.after_each(range(len(refs_new)), range(first, first + len(fams))) + \
            cs.after_each(range(len(refs_new), first), range(first + N_OLD, first + len(fams)))
        assert len(refs_new) == (16 if env.device else 25) and len(refs_old) >= (50 if env.device else 80)
        assert len(plan) == 2 * (len(refs_new) * 45 + len(refs_old) * 10)
        assert {every[r].entry for r in plan[0::2]} >= {f.entry for f in fams if set(f.modes) - {"fit", "decreasing"}}
        assert cs.run(plan, every, _refusal_sizes(plan, every)) == len(plan)


@POINTERS
def test_rules_do_not_leak_into_or_out_of_the_new_families(gpu, oracle, pointers):
    """every later family that cuts at latok's boundaries straight after latok_set_rules(all_columns) and straight after
    latok_reset_rules, a family that reads no rule between each pair; and the same for the three that must NOT change: the pre-tokens,
    the BPE ids on them and the decoder hold, behind latok_set_rules, what they hold under the built-in rules ("latok_set_rules has no
    influence")"""
    with _Session(gpu, oracle, pointers) as env:
        fams = _all_families(env)
        fold = next(i for i, f in enumerate(fams) if f.entry == "latok_fold_utf8_bytes_batch")
        csr = next(i for i, f in enumerate(fams) if f.entry == "latok_tfidf_csr")
        every = fams + [Rules(env, "all_columns"), Rules(env, None)]
        on, off = len(fams), len(fams) + 1
        plan, n_boundary, n_free = [], 0, 0
        for i in NEW:
            if fams[i].boundary or fams[i].entry in RULE_FREE_NEW:
                k = n_boundary + n_free
                plan += [on, i, fold if k % 2 else csr, off, i, csr if k % 2 else fold]
                n_boundary, n_free = n_boundary + fams[i].boundary, n_free + (not fams[i].boundary)
        assert (n_boundary, n_free) == (6, 3)
        B = _batches()
        shapes = [("M5", cs.DENSE), ("M", cs.SPARSE), ("S", cs.DENSE), ("S600", cs.SPARSE)]
        sizes = [B[shapes[(k // 3) % len(shapes)]] for k in range(len(plan))]
        # the tables do change the tokens of these batches: else the six boundary families would show nothing
        assert any(not np.array_equal(cs.reference(oracle, b).byte_spans, cs.reference(oracle, b, RULE_SETS["all_columns"], "cps", "all_columns").byte_spans)
                   for b in sizes)
        assert cs.run(plan, every, sizes) == len(plan) == 6 * 9


def test_new_families_on_rotating_caller_streams(gpu, oracle):
    """device pointers, the touching plan, step k on stream k % 3 of {NULL, s1, s2}; an asynchronous call of the 35 is read only after
    the later family behind it has been enqueued"""
    with _Session(gpu, oracle, "device") as env:
        hip = env.lib
        s1, s2 = C.c_void_p(), C.c_void_p()
        assert hip.hipStreamCreate(C.byref(s1)) == 0 and hip.hipStreamCreate(C.byref(s2)) == 0
        try:
            env.streams, env.defer, env.keep = [None, s1, s2], True, True
            fams = _all_families(env)
            plan, sizes = _touching_plan(fams)
            used = set()
            assert cs.run(plan, fams, sizes, on_step=lambda k, f, b, o: used.add((f.name, (k % 3)))) == 801
            assert used == {(fams[f].name, k % 3) for k, f in enumerate(plan)}
            assert all(sum((fams[f].name, s) in used for s in range(3)) == 3 for f in NEW)       # every later family on all three streams
            assert sum(fams[a].asynchronous and b >= N_OLD for a, b in cs.pairs_of(plan)) == 6 * N_NEW      # each read behind a later family
            assert hip.hipStreamSynchronize(s1) == 0 and hip.hipStreamSynchronize(s2) == 0
            env._lib.check(env.lib.latok_sync())
        finally:
            env.streams = None
            hip.hipStreamDestroy(s1)
            hip.hipStreamDestroy(s2)


@POINTERS
def test_scan_epoch_wrap_inside_the_new_multi_scan_calls(gpu, oracle, pointers):
    """the 18-bit scan epoch wraps between two scans of one call: each later multi-scan family starts four epochs in front of the wrap at
    M5, then one full turn of all 45 families"""
    with _Session(gpu, oracle, pointers) as env:
        fams = _all_families(env)
        B = _batches()
        gpu.latok_debug_set_scan_epoch.restype, gpu.latok_debug_set_scan_epoch.argtypes = C.c_int, [C.c_uint]
        for start in (0x3FFFE, 0x3FFFF, 0x3FFFD, 0x3FFFC):
            for name in NEW_MULTI_SCAN:
                i = next(i for i, f in enumerate(fams) if f.name == name)
                assert gpu.latok_debug_set_scan_epoch(start) == 0
                assert cs.run([i, i], fams, [B[("M5", cs.DENSE)], B[("M5", cs.SPARSE)]]) == 2
        assert gpu.latok_debug_set_scan_epoch(0x3FFFC) == 0
        turn = list(range(len(fams)))
        keys = cs.rotation(turn, [f.uses_l for f in fams])
        assert cs.run(turn, fams, [B[k] for k in keys]) == 45
