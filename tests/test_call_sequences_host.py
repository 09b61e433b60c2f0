"""The plans, the batches, the references and the driver of tests/test_gpu_call_sequences.py, without a GPU.

* the plans cover what they claim: every ordered pair, every (refusal, family) pair, a DENSE-then-SPARSE step of non-increasing length in
  front of every family, L in at most one step of eight and only for the families that take it;
* the driver judges: fed fake families -- one stateless, one that is wrong only behind a named family at a named size, one that is wrong
  only on its second occurrence after a refusal, one whose result is read late -- it fails on exactly that step and names predecessor,
  family, size, array and index, and it passes the all-correct plan.  That is the proof that the GPU test sees an order-dependent error;
* the batches have the shapes the issue names, relative to the library's own thresholds (latok_debug_limits needs no device);
* every family's expectation can be computed here, for every batch it gets;
* for the ten families that came after the 35: the touching plan holds every ordered pair with one of them in it exactly once and no
  other, the rotation serves it, their expectations have the right arrays, shapes and dtypes, follow the rule tables exactly where the
  family cuts at latok's boundaries, and none is vacuous -- unk pieces, merged pieces, marked and unmarked Unigram pieces, unknown and
  skipped ids, out-of-vocabulary grams are all there on both contents of M5."""
import time

import numpy as np
import pytest

from helpers import call_sequences as cs

import test_gpu_call_sequences as seq

N_FAMILIES = 35


# ---- plans ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, N_FAMILIES])
def test_pair_cover_holds_every_ordered_pair(n):
    plan = cs.pair_cover(n)
    assert len(plan) == n * n + 1 and plan[0] == plan[-1]
    pairs = cs.pairs_of(plan)
    assert len(pairs) == n * n and set(pairs) == {(a, b) for a in range(n) for b in range(n)}
    assert plan == cs.pair_cover(n)                                          # deterministic
    with pytest.raises(ValueError):
        cs.pair_cover(0)


def test_after_each_puts_every_family_behind_every_refusal():
    refusers, families = list(range(100, 107)), list(range(N_FAMILIES))
    plan = cs.after_each(refusers, families)
    assert len(plan) == 2 * 7 * N_FAMILIES and plan == cs.after_each(refusers, families)
    assert plan[0::2] == [r for r in refusers for _ in families]
    assert set(zip(plan[0::2], plan[1::2])) == {(r, f) for r in refusers for f in families}


def test_rotation_puts_a_sparse_batch_behind_a_longer_dense_one_in_front_of_every_family():
    env = seq.Env(None, None, False)
    fams = seq._families(env)
    uses_l = [f.uses_l for f in fams]
    assert sum(uses_l) == 12                                                 # the UTF-32, kind and code-point families
    plan = cs.pair_cover(N_FAMILIES)
    keys = cs.rotation(plan, uses_l)
    assert keys == cs.rotation(plan, uses_l) and len(keys) == len(plan)
    B = seq._batches()
    seen, sizes_of, streams_of = set(), {}, {}
    for k in range(1, len(plan)):
        (s0, c0), (s1, c1) = keys[k - 1], keys[k]
        if c0 == cs.DENSE and c1 == cs.SPARSE and B[(s0, c0)].total_bytes >= B[(s1, c1)].total_bytes and B[(s0, c0)].total_bytes > 0:
            seen.add(plan[k])
    assert seen == set(range(N_FAMILIES))
    for k, f in enumerate(plan):
        sizes_of.setdefault(f, set()).add(keys[k])
        streams_of.setdefault(f, set()).add(k % 3)
        assert keys[k][0] != "L" or uses_l[f]
    n_l = sum(1 for s, _ in keys if s == "L")
    assert 0 < n_l <= len(plan) // 8
    assert all(len(v) >= 6 for v in sizes_of.values())                       # no family is pinned to one batch
    assert all(any(s == "L" for s, _ in sizes_of[f]) for f in range(N_FAMILIES) if uses_l[f])
    # step k runs on stream k % 3: every family meets at least two of the three streams, all but three of them all three
    assert all(len(v) >= 2 for v in streams_of.values()) and sum(len(v) == 3 for v in streams_of.values()) >= N_FAMILIES - 3
    # int32 and int64 occurrences of every family meet both contents
    occ, met = {}, set()
    for k, f in enumerate(plan):
        met.add((f, occ.get(f, 0) % 2, keys[k][1]))
        occ[f] = occ.get(f, 0) + 1
    assert len(met) == 4 * N_FAMILIES


# ---- the driver's judgement ----------------------------------------------------------------------------------------------------------
class World:
    def __init__(self):
        self.last, self.refused, self.expects = None, False, []


class Fake:
    """a correct family: its result is a function of the batch alone"""
    stateful = False

    def __init__(self, world, name):
        self.world, self.name = world, name

    def truth(self, batch):
        n = 5 + len(batch)
        return {"counts": np.arange(n, dtype=np.int64), "items": np.arange(2 * n, dtype=np.int64).reshape(n, 2) * 3}

    def wrong(self, batch, occ):
        return False

    def call(self, batch, occ):
        res = self.truth(batch)
        if self.wrong(batch, occ):
            res["items"] = res["items"].copy()
            res["items"][3, 1] += 1
        self.world.last = (self.name, batch)
        if occ % 2:
            res = {k: v.astype(np.int32) for k, v in res.items()}            # the narrow width holds the same values
        return res

    def expect(self, batch):
        self.world.expects.append((self.name, batch))
        return self.truth(batch)


class WrongBehind(Fake):
    """wrong only when the step before it was ``pred`` on ``pred_batch``: a plane the predecessor left dirty"""

    def __init__(self, world, name, pred, pred_batch):
        super().__init__(world, name)
        self.trigger = (pred, pred_batch)

    def wrong(self, batch, occ):
        return self.world.last == self.trigger


class Refuser(Fake):
    def call(self, batch, occ):
        self.world.refused = True
        self.world.last = (self.name, batch)
        return {"rc": np.array([-1])}

    def expect(self, batch):
        return {"rc": np.array([-1])}


class WrongSecondTimeAfterRefusal(Fake):
    """wrong only on its second occurrence behind a refusal: a pinned word the refused call left set and the first call half-cleared"""

    def __init__(self, world, name):
        super().__init__(world, name)
        self.after = 0

    def wrong(self, batch, occ):
        if self.world.last and self.world.last[0].startswith("refuse"):
            self.after += 1
            return self.after == 2
        return False


class Late(Fake):
    """an asynchronous family: the result is handed over when the driver asks, which must be after the next step was enqueued"""

    def __init__(self, world, name, wrong_at=None):
        super().__init__(world, name)
        self.wrong_at, self.asked_after = wrong_at, []

    def wrong(self, batch, occ):
        return occ == self.wrong_at

    def call(self, batch, occ):
        res = super().call(batch, occ)
        mine = self.world.last

        def later():
            self.asked_after.append(self.world.last != mine)
            return res
        return later


def _fakes(world, bad=None):
    fams = [Fake(world, "f%d" % i) for i in range(7)]
    if bad is not None:
        fams[bad.slot] = bad
    return fams


def _sizes(plan):
    names = ["S/DENSE", "M/SPARSE", "M5/DENSE", "E/SPARSE", "S600/DENSE"]
    return [names[k % len(names)] for k in range(len(plan))]


def test_driver_passes_the_correct_plan_and_asks_for_each_expectation_once():
    world = World()
    fams = _fakes(world)
    plan = cs.pair_cover(7)
    assert cs.run(plan, fams, _sizes(plan)) == 50
    per_key = {}
    occ = {}
    for k, f in enumerate(plan):
        per_key.setdefault((fams[f].name, _sizes(plan)[k], occ.get(f, 0) % 2), 0)
        occ[f] = occ.get(f, 0) + 1
    assert len(world.expects) == len(per_key)                                # once per (family, batch, width)
    with pytest.raises(ValueError):
        cs.run(plan, fams, _sizes(plan)[:-1])                                # a shortened list of batches is no plan


def test_driver_names_the_step_behind_a_named_predecessor():
    world = World()
    plan = cs.pair_cover(7)
    sizes = _sizes(plan)
    k_bad = next(k for k in range(1, len(plan)) if plan[k] == 4 and plan[k - 1] == 2)
    bad = WrongBehind(world, "f4", "f2", sizes[k_bad - 1])
    bad.slot = 4
    # the pair (f2, f4) occurs once in the plan; f4 behind any other family, or behind f2 on another batch, is right
    with pytest.raises(cs.SequenceError) as e:
        cs.run(plan, _fakes(world, bad), sizes)
    err = e.value
    assert (err.step, err.pred, err.pred_batch, err.family, err.batch) == (k_bad, "f2", sizes[k_bad - 1], "f4", sizes[k_bad])
    assert err.array == "items" and err.index == (3, 1) and err.got == err.want + 1
    assert err.width == cs.WIDTHS[sum(1 for f in plan[:k_bad] if f == 4) % 2]
    for part in ("step %d" % k_bad, "f2", "f4", sizes[k_bad], sizes[k_bad - 1], "items", "(3, 1)"):
        assert part in str(err)
    # the same fake behind the same family on ANOTHER batch: no error, the plan passes
    world = World()
    other = WrongBehind(world, "f4", "f2", "no such batch")
    other.slot = 4
    assert cs.run(plan, _fakes(world, other), sizes) == 50


def test_driver_names_the_second_occurrence_behind_a_refusal():
    world = World()
    bad = WrongSecondTimeAfterRefusal(world, "f5")
    bad.slot = 5
    fams = _fakes(world, bad)
    refusers = [Refuser(world, "refuse%d" % i) for i in range(3)]
    every = refusers + fams
    plan = cs.after_each(range(3), range(3, 10))
    sizes = _sizes(plan)
    with pytest.raises(cs.SequenceError) as e:
        cs.run(plan, every, sizes)
    k_bad = [k for k in range(len(plan)) if every[plan[k]].name == "f5"][1]
    err = e.value
    assert (err.step, err.family, err.pred, err.batch, err.pred_batch) == (k_bad, "f5", "refuse1", sizes[k_bad], sizes[k_bad - 1])
    assert err.array == "items" and err.index == (3, 1)
    world = World()
    assert cs.run(plan, [Refuser(world, "refuse%d" % i) for i in range(3)] + _fakes(world), sizes) == len(plan)


def test_driver_reads_an_asynchronous_result_after_the_next_step_and_blames_its_own_step():
    world = World()
    late = Late(world, "f3", wrong_at=2)
    late.slot = 3
    plan = cs.pair_cover(7)
    sizes = _sizes(plan)
    with pytest.raises(cs.SequenceError) as e:
        cs.run(plan, _fakes(world, late), sizes)
    k_bad = [k for k in range(len(plan)) if plan[k] == 3][2]
    assert (e.value.step, e.value.family, e.value.batch, e.value.pred) == (k_bad, "f3", sizes[k_bad], "f%d" % plan[k_bad - 1])
    assert late.asked_after == [True, True, True]                            # each result was asked for behind the following call
    world = World()
    ok = Late(world, "f6")
    ok.slot = 6
    assert cs.run(plan, _fakes(world, ok), sizes) == 50                      # the closing step is f0: nothing is left unread
    assert len(ok.asked_after) == 7 and all(ok.asked_after)
    world = World()
    last = Late(world, "f0", wrong_at=7)                                     # the plan's last step: read when the plan ends
    last.slot = 0
    with pytest.raises(cs.SequenceError) as e:
        cs.run(plan, _fakes(world, last), sizes)
    assert e.value.step == len(plan) - 1


def test_first_difference_and_approx():
    a = np.arange(6, dtype=np.int64)
    assert cs.first_difference(a.astype(np.int32), a) is None
    assert cs.first_difference(a[:5], a) == ("shape", (5,), (6,))
    b = a.copy()
    b[4] = -1
    assert cs.first_difference(b, a) == (4, -1, 4)
    m = np.array([1, 2 ** 63 + 5], np.uint64)
    assert cs.first_difference(m, m.copy()) is None and cs.first_difference(m, np.array([1, 5], np.uint64))[0] == 1
    want = cs.Approx([1.0, 0.0, -2.0], [1e-6, 1e-6, 1e-6])
    assert want.first_difference(np.array([1.0 + 5e-7, 0.0, -2.0], np.float32)) is None
    assert want.first_difference(np.array([1.0, 1e-30, -2.0], np.float32))[0] == 1       # zero means zero
    assert want.first_difference(np.array([1.0, 0.0, np.nan], np.float32))[0] == 2
    assert want.first_difference(np.array([1.00001, 0.0, -2.0], np.float32))[0] == 0


# ---- the batches ---------------------------------------------------------------------------------------------------------------------
def test_batches_have_the_shapes_the_routes_turn_on(oracle):
    tile, small_chars, small_strings = seq._limits()
    B = seq._batches()
    assert set(B) == {(s, c) for s in cs.SIZE_NAMES for c in (cs.DENSE, cs.SPARSE)}
    again = cs.build_batches(tile, small_chars, small_strings)
    for key, b in B.items():
        assert np.array_equal(b.u8, again[key].u8) and np.array_equal(b.boff, again[key].boff), key          # fixed seeds
    for c in (cs.DENSE, cs.SPARSE):
        e, s, s600, sn, m, m5, big = (B[(x, c)] for x in cs.SIZE_NAMES)
        assert e.n_str == 3 and e.total_bytes == 0
        assert s.n_str == 1 and s.total_bytes == 37                                      # ends inside the first 64-bit word
        assert s600.n_str == 600 and s600.total_bytes < tile
        assert sn.n_str == small_strings + 1 and sn.total_bytes == s600.total_bytes      # one string too many for the pinned small route
        assert m.n_str == 9 and m.total_bytes == tile + 37
        assert 60 <= m5.n_str <= 80 and m5.total_bytes == 5 * tile + 11
        assert small_chars < big.total_chars <= small_chars + 64 and big.total_bytes > small_chars
        for b in (s, s600, sn, m, m5, big):
            assert b.total_bytes % 64 and b.total_chars % 64, b.key                      # the end is not on a word edge
            raw = b.u8.tobytes()
            cut = [i for i in range(b.n_str) if raw[b.boff[i]:b.boff[i + 1]].endswith(cs.CUT)]
            assert len(cut) == 1, b.key                                                  # the one malformed string
            nxt = raw[b.boff[cut[0] + 1]:b.boff[cut[0] + 1] + 1]
            assert nxt == b"" or nxt[0] < 0x80                                           # what follows it is no continuation byte
            for i in range(b.n_str):
                if i != cut[0]:
                    raw[b.boff[i]:b.boff[i + 1]].decode("utf-8")                         # everything else is well-formed
            assert 0xFFFD in b.cps and b.k1.max() <= 0xFF and b.k2.dtype == np.uint16
            assert (b.cps >= 0x10000).any() == (c == cs.DENSE) or b.size == "S"
        # the M batch: a token lies across the tile edge
        r = cs.reference(oracle, m)
        a = r.byte_spans[:, 0] + m.boff[r.tok_str]
        z = r.byte_spans[:, 1] + m.boff[r.tok_str]
        assert ((a < tile) & (z > tile)).any(), c
        r5 = cs.reference(oracle, m5)
        a, z = r5.byte_spans[:, 0] + m5.boff[r5.tok_str], r5.byte_spans[:, 1] + m5.boff[r5.tok_str]
        assert any(((a < t * tile) & (z > t * tile)).any() for t in range(1, 6)), c
    # DENSE leaves every plane full: about one boundary per two bytes, every token of one char, in the vocabulary
    d, sp = cs.reference(oracle, B[("M5", cs.DENSE)]), cs.reference(oracle, B[("M5", cs.SPARSE)])
    assert d.n_tokens > B[("M5", cs.DENSE)].total_bytes * 0.45 and d.n_tokens > 8 * sp.n_tokens
    in_vocab = sum(t in seq.VOCAB for t in d.tokens)
    assert in_vocab > 0.97 * d.n_tokens
    assert (np.diff(d.byte_spans, axis=1) >= 2).any()                                    # 2-, 3- and 4-byte letters among them
    # SPARSE: long words, some out of vocabulary, runs of empty strings, a row of marks only
    oov = sum(t not in seq.VOCAB for t in sp.tokens)
    assert 0 < oov < sp.n_tokens and np.diff(sp.byte_spans, axis=1).mean() > 8
    m5 = B[("M5", cs.SPARSE)]
    lens = np.diff(m5.boff)
    assert any((lens[i:i + 3] == 0).all() for i in range(m5.n_str - 3))
    assert any(bytes(m5.blobs[i]) == "́́́".encode("utf-8") for i in range(m5.n_str))
    # the strip rule of the reference is str.strip(): the SPACE column agrees with str.isspace on every char of every batch
    for b in B.values():
        if b.total_chars:
            space = cs.reference(oracle, b).matrix[:, 5] != 0
            uniq, first = np.unique(b.cps, return_index=True)
            for cp, i in zip(uniq.tolist(), first.tolist()):
                assert chr(cp).isspace() == bool(space[i]), hex(cp)


def test_reference_agrees_with_the_oracle_string_by_string(oracle):
    """the vectorised reference against oracle.tokenize / split_offsets, one string at a time, on the well-formed strings of M5"""
    for c in (cs.DENSE, cs.SPARSE):
        b = seq._batches()[("M5", c)]
        r = cs.reference(oracle, b)
        rows = r.rows()
        k = 0
        for s in range(b.n_str):
            text = "".join(map(chr, b.cps[b.row[s]:b.row[s + 1]].tolist()))
            n_off = int(r.off_counts[s])
            if text:
                assert r.offsets[k:k + n_off].tolist() == oracle.split_offsets(text).tolist(), s
                if "�" not in text:
                    assert [t.decode("utf-8") for t in rows[s]] == oracle.tokenize(text), s
            else:
                assert n_off == 0 and rows[s] == []
            k += n_off
        assert k == r.offsets.size


# ---- every family's expectation --------------------------------------------------------------------------------------------------------
def test_every_expectation_is_computable_here(oracle, capsys):
    env = seq.Env(None, oracle, False)
    fams = seq._families(env)
    assert [f.entry for f in fams] == [name for name, _ in seq._makers()] and len(fams) == N_FAMILIES
    B = seq._batches()
    t_l = {}
    for f in fams:
        for (size, content), b in B.items():
            if size == "L" and not f.uses_l:
                continue
            for odd in (0, 1):
                f.occ = f.odd = odd
                t0 = time.perf_counter()
                want = f.expect(b)
                if size == "L":
                    t_l[f.entry] = t_l.get(f.entry, 0.0) + time.perf_counter() - t0
                assert want["rc"].tolist() == [0] and len(want) >= 2, (f.name, b.key)
                for name, v in want.items():
                    assert isinstance(v, (np.ndarray, cs.Approx)), (f.name, name)
    with capsys.disabled():
        print("\nseconds for the L expectations (both contents, both widths; the batch's reference is shared): " +
              ", ".join("%s %.2f" % (k.replace("latok_", ""), v) for k, v in sorted(t_l.items())))
    # the refusing forms of every family: each names its mode, and there are as many as the GPU test counts on
    assert len(seq._refusers(env)) >= 80
    env.device = True
    assert len(seq._refusers(env)) >= 50


# ---- the ten later families: the touching plan, their expectations ---------------------------------------------------------------------
N_ALL = N_FAMILIES + 10
NEW = range(N_FAMILIES, N_ALL)


@pytest.mark.parametrize("n, new", [(N_ALL, tuple(NEW)), (5, (4,)), (3, (0, 1, 2)), (6, (0, 3)), (1, (0,)), (9, (2, 7, 8))])
def test_pair_cover_touching_holds_every_pair_with_a_new_member_once(n, new):
    plan = cs.pair_cover_touching(n, new)
    want = {(a, b) for a in range(n) for b in range(n) if a in new or b in new}
    assert len(want) == n * n - (n - len(new)) ** 2
    pairs = cs.pairs_of(plan)
    assert len(plan) == len(want) + 1 and plan[0] == plan[-1]
    assert len(pairs) == len(set(pairs)) and set(pairs) == want                # each required pair once, and no pair of two old ones
    assert plan == cs.pair_cover_touching(n, list(reversed(new)))              # deterministic, whatever the order of ``new``
    if len(new) == n:
        assert set(pairs) == set(cs.pairs_of(cs.pair_cover(n)))
    for bad in ((), (n,), (-1,)):
        with pytest.raises(ValueError):
            cs.pair_cover_touching(n, bad)


def test_touching_plan_of_the_45_has_800_pairs_and_801_steps():
    plan = cs.pair_cover_touching(N_ALL, NEW)
    assert len(plan) == 801 and len(set(cs.pairs_of(plan))) == 800 == N_ALL ** 2 - N_FAMILIES ** 2
    assert not any(a < N_FAMILIES and b < N_FAMILIES for a, b in cs.pairs_of(plan))


def test_rotation_puts_a_sparse_batch_behind_a_longer_dense_one_in_front_of_every_new_family():
    env = seq.Env(None, None, False)
    fams = seq._all_families(env)
    uses_l = [f.uses_l for f in fams]
    assert sum(uses_l) == 12 and not any(uses_l[f] for f in NEW)             # the later families are all byte-space
    plan, sizes = seq._touching_plan(fams)
    keys = cs.rotation(plan, uses_l)
    assert [b.key for b in sizes] == ["%s/%s" % k for k in keys]
    B = seq._batches()
    seen, sizes_of, streams_of = set(), {}, {}
    for k in range(1, len(plan)):
        (s0, c0), (s1, c1) = keys[k - 1], keys[k]
        if c0 == cs.DENSE and c1 == cs.SPARSE and B[(s0, c0)].total_bytes >= B[(s1, c1)].total_bytes and B[(s0, c0)].total_bytes > 0:
            seen.add(plan[k])
    assert seen >= set(NEW)
    for k, f in enumerate(plan):
        sizes_of.setdefault(f, set()).add(keys[k])
        streams_of.setdefault(f, set()).add(k % 3)
        assert keys[k][0] != "L" or uses_l[f]
    assert all(len(sizes_of[f]) >= 6 and len(streams_of[f]) == 3 for f in NEW)
    # int32 and int64 occurrences of every later family meet both contents; each meets the dense M5 and a sparse batch of several tiles
    occ, met = {}, set()
    for k, f in enumerate(plan):
        met.add((f, occ.get(f, 0) % 2, keys[k][1]))
        occ[f] = occ.get(f, 0) + 1
    assert all((f, odd, c) in met for f in NEW for odd in (0, 1) for c in (cs.DENSE, cs.SPARSE))
    assert all(("M5", cs.DENSE) in sizes_of[f] and {("M", cs.SPARSE), ("M5", cs.SPARSE)} & sizes_of[f] for f in NEW)     # (more than a tile)


SHAPES = {"indptr": 1, "oov": 1, "indices": 1, "data": 1, "ids": 1, "spans": 2, "items": 2, "counts": 1, "input_ids": 2, "lengths": 1, "bytes": 1,
          "out_off": 1}
DTYPES = {"indices": np.int32, "data": np.int32, "ids": np.int32, "input_ids": np.int32, "lengths": np.int32, "bytes": np.uint8, "out_off": np.int64}


def test_every_new_expectation_is_computable_here(oracle):
    """every later family's expect(), on the CPU, for every batch it can meet, in both widths and under the rule tables: the right
    arrays, shapes and dtypes; and none of them is vacuous on M5"""
    env = seq.Env(None, oracle, False)
    fams = seq._all_families(env)[N_FAMILIES:]
    assert [f.name for f in fams] == [name for name, _ in seq._new_makers()] and len(fams) == 10
    B = seq._batches()
    for f in fams:
        for (size, content), b in B.items():
            if size == "L":
                assert not f.uses_l
                continue
            for odd in (0, 1):
                f.occ = f.odd = odd
                want = f.expect(b)
                assert want["rc"].tolist() == [0] and set(want) - {"rc", "guard bytes overwritten"} <= set(SHAPES) | {"n", "nnz", "total", "n_pieces",
                                                                                                                  "n_tokens", "n_unknown"}
                for name, v in want.items():
                    assert isinstance(v, np.ndarray), (f.name, name)
                    if name in SHAPES:
                        assert v.ndim == SHAPES[name] and v.dtype == DTYPES.get(name, np.int64), (f.name, b.key, name, v.dtype, v.shape)
                rows = next(want[k] for k in ("indptr", "out_off", "counts", "lengths") if k in want)
                assert rows.shape[0] == b.n_str + (0 if rows is want.get("counts") or rows is want.get("lengths") else 1), (f.name, b.key)
                for rec, total in (("indices", "nnz"), ("data", "nnz"), ("ids", "n_pieces"), ("spans", "n_pieces"), ("items", "n"), ("bytes", "n")):
                    if rec in want:
                        assert want[rec].shape[0] == int(want[total][0]) == int(rows.sum() if rows.shape[0] == b.n_str else rows[-1]), (f.name, b.key, rec)
                if "input_ids" in want:
                    assert want["input_ids"].shape == (b.n_str, seq.PIECE_LEN) and (want["lengths"] >= 2).all() and (want["lengths"] <= seq.PIECE_LEN).all()
    # the refusing forms, and the boundary families under the rule tables: other tokens, so another expectation
    assert len(seq._refusers(env, seq._new_makers())) == 25
    env.device = True
    assert len(seq._refusers(env, seq._new_makers())) == 16
    env.device = False
    m5 = B[("M5", cs.DENSE)]
    for odd in (0, 1):
        plain = {}
        for f in fams:
            f.occ = f.odd = odd
            plain[f.name] = f.expect(m5)
        env.rules = "all_columns"
        for f in fams:
            f.occ = f.odd = odd
            ruled = f.expect(m5)
            same = all(cs.first_difference(ruled[k], plain[f.name][k]) is None for k in ruled)
            # (the padded BPE call takes the latok-token object on even occurrences and GPT-2's pre-tokens on odd ones)
            assert same == (not f.boundary or (f.name == "latok_bpe_padded_utf8_bytes_batch" and odd == 1)), (f.name, odd)
        env.rules = None
    env.rules = None


def test_no_new_expectation_is_vacuous(oracle):
    """from the reference alone, on both contents of M5: BPE leaves an unk piece and a piece of several bytes, on either front; Unigram a
    piece behind the marker and one without; both decoders meet an id they do not hold and ids they skip; the char-gram CSR has entries and
    grams that are not in the vocabulary"""
    env = seq.Env(None, oracle, False)
    inverse = {i: w for w, i in seq.UNI_DICT.items()}
    for c in (cs.DENSE, cs.SPARSE):
        b = seq._batches()[("M5", c)]
        for kind in ("bpe", "gpt2"):
            _, ids, spans, n_tok = seq._pieces(env, b, kind)
            width = spans[:, 1] - spans[:, 0]
            assert (ids == seq.BPE_UNK).any() and ((ids != seq.BPE_UNK) & (width > 1)).any() and ids.size > n_tok > 0, (c, kind)
        over = (np.diff(cs.reference(oracle, b).byte_spans, axis=1) > seq.PIECE_MAX_BYTES).any()
        assert over == (c == cs.SPARSE)                                       # the over-long tokens are the SPARSE batch's
        _, ids, spans, _ = seq._pieces(env, b, "uni")
        words = [inverse.get(int(i)) for i in ids]
        assert any(w is not None and w.startswith(seq.unigram_ref.MARKER) for w in words), c
        assert any(w is not None and not w.startswith(seq.unigram_ref.MARKER) for w in words) and (ids == seq.UNI_UNK).any(), c
        assert (spans[:, 1] == spans[:, 0]).any() or c == cs.SPARSE           # the marker alone: an empty range
        for fam in (seq.DetokCsr(env), seq.DetokPadded(env)):
            for odd in (0, 1):
                fam.occ = fam.odd = odd
                want = fam.full(b)
                assert want["n_unknown"] > 0 and want["n"] > 0, (c, fam.name, odd)
        for odd, (kind, skip) in enumerate((("bpe", seq.DETOK_BPE_SKIP), ("wp", seq.DETOK_WP_SKIP))):
            ids = seq._pieces(env, b, kind, rules=False)[1]
            assert any((ids == s).any() for s in skip), (c, kind)
        for odd in (0, 1):
            fam = seq.CharGrams(env, "fit", "latok_chargram_counts_utf8_bytes_batch", False)
            fam.occ = fam.odd = odd
            want = fam.full(b)
            assert want["oov"].sum() > 0 and (want["data"] > 0).any() and want["nnz"] > 0 and want["total"] > want["oov"].sum(), (c, odd)
            fam = seq.CharGrams(env, "fit", "latok_hashed_chargram_counts_utf8_bytes_batch", True)
            fam.occ = fam.odd = odd
            want = fam.full(b)
            assert (want["data"] != 0).any() and ((want["data"] < 0).any() == bool(odd)), (c, odd)


def test_the_memoised_cut_is_the_helpers_cut(oracle):
    """seq._cut_rows cuts every distinct token once; bpe_ref.cut_rows, unigram_ref.cut_rows and wordpiece_ref.cut_rows cut each where it
    stands: the same rows.  And the vectorised padded block is the rows written out one by one"""
    env = seq.Env(None, oracle, False)
    for key in (("M5", cs.DENSE), ("M5", cs.SPARSE), ("S600", cs.DENSE), ("M", cs.SPARSE)):
        b = seq._batches()[key]
        r = cs.reference(oracle, b)
        counts, spans = seq._pretok(b)
        want = {"bpe": seq.bpe_ref.cut_rows(b.u8, b.boff, r.counts, r.byte_spans.tolist(), seq.BPE_DICT, seq.PIECE_MAX_BYTES, True, seq.BPE_UNK),
                "gpt2": seq.bpe_ref.cut_rows(b.u8, b.boff, counts, spans.tolist(), seq.GPT2_DICT, seq.PIECE_MAX_BYTES, False, seq.BPE_UNK),
                "uni": seq.unigram_ref.cut_rows(b.u8, b.boff, r.counts, r.byte_spans.tolist(), seq.UNI_DICT, seq.UNI_SCORES, seq.UNI_UNK_SCORE,
                                                seq.unigram_ref.MARKER, True, seq.PIECE_MAX_BYTES, seq.UNI_UNK),
                "wp": seq.wpr.cut_rows(b.u8, b.boff, r.counts, r.byte_spans.tolist(), seq.WP_DICT, cs.WP_PREFIX, 100, seq.DETOK_WP_UNK)}
        for kind, (indptr, ids, sp) in want.items():
            got = seq._pieces(env, b, kind)
            assert got[0].tolist() == list(indptr) and got[1].tolist() == list(ids), (key, kind)
            assert got[2].tolist() == [list(x) for x in np.asarray(sp).reshape(-1, 2).tolist()], (key, kind)
            if kind != "wp":
                rows, lengths = seq._padded(got[0], got[1], b.n_str, 91, 92, 93)
                for s in range(b.n_str):
                    row = [91] + list(ids[indptr[s]:indptr[s + 1]])[:seq.PIECE_LEN - 2] + [92]
                    assert rows[s].tolist() == row + [93] * (seq.PIECE_LEN - len(row)) and lengths[s] == len(row), (key, kind, s)
        # every pre-token range lies in its string, and together they cover it
        assert counts.sum() == spans.shape[0] and (spans[:, 1] > spans[:, 0]).all()
        assert int((spans[:, 1] - spans[:, 0]).sum()) == b.total_bytes
