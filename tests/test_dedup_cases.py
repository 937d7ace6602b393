"""The generators of tests/dedup_cases.py keep their promises, under the oracle alone (no GPU): the restatement `model` equals
loader.regs_finish region by region on every batch the GPU tests run; every tagged pair reaches the alignment, goes through the
named statement of it and ends on the named side of the threshold; every tier meets enough events of every kind; the pairs of
the rounding edge are told apart by contraction, and the oracle decides as the uncontracted expression does.  These are
conditions on the inputs, not measurements of the library: tests/test_gpu_dedup_limits.py compares the device's counts with the
numbers checked here."""
import collections

import numpy as np
import pytest

import aln_cases as ac
import dedup_cases as dc
from oracle import loader
from util import toy


@pytest.fixture(scope="module")
def env():
    g, idx = toy()
    return g, idx.ref_0123, dc.contigs_of(len(g))


def _model(env, c, okw, force_seq=False):
    """The model of the batch, after holding it against the oracle."""
    g, ref, contigs = env
    oopt = ac.opts(**okw)[0]
    enc, cum, regs, off = c.flat()
    want, woff = loader.regs_finish(regs, off, enc, cum, ref, len(g), contigs=contigs, opt=oopt)
    m = dc.model(oopt, regs, off, enc, cum, ref, len(g), contigs, force_seq)
    out = [x for st in m for x in st["out"]]
    assert np.array_equal(np.concatenate([[0], np.cumsum([len(st["out"]) for st in m])]), woff)
    assert out == [tuple(int(want[i][f]) for f in dc.FIELDS) for i in range(len(want))]
    return m


def _pairs(c, m, tag):
    """The candidates of the reads with this tag: exactly one each (the pair), at least 8 in all."""
    xs = [st["cands"] for t, st in zip(c.tags, m) if t == tag]
    assert len(xs) >= 8 and all(len(x) == 1 for x in xs), (tag, [len(x) for x in xs])
    return [x[0] for x in xs]


@pytest.mark.parametrize("okw", dc.OPTS, ids=("default", "alt"))
def test_variant_pairs(env, okw):
    g = env[0]
    opt = ac.opts(**okw)[0]
    reg_of = {63: "reg1", 64: "reg2", 127: "reg2", 128: "reg3", 191: "reg3", 192: "reg4", 255: "reg4", 256: "lds", 999: "lds"}
    for pad, long_read in ((0, False), (dc.PAD, False), (dc.PAD, True)):
        c = dc.variant_cases(g, opt, pad, long_read)
        m = _model(env, c, okw)
        assert all(st["tier"] == ("lane" if pad == 0 else "wave128") for st, t in zip(m, c.tags) if t != "long")
        for lq, v in reg_of.items():
            ps = _pairs(c, m, "lq%d" % lq)
            assert all(x["lq"] == lq and x["merged"] and x["variant"] == (v if pad and not long_read else "hbm") for x in ps), lq
            # the band at its floor dl + 3 and capped by 4 opt.w on the way (the merged region's w says which)
            assert sum(x["band"] == abs(x["rlen"] - x["lq"]) + 3 for x in ps) >= 2 and sum(x["band"] > abs(x["rlen"] - x["lq"]) + 3 for x in ps) >= 2
        assert {st["out"][0][dc.FIELDS.index("w")] for st, t in zip(m, c.tags) if t.startswith("lq")} >= {opt.w << 2, 10}
        assert all(x["variant"] == "shortcut" and x["merged"] for x in _pairs(c, m, "shortcut"))
        for tag in ("short_w1", "short_len1", "n"):
            assert all(x["variant"] not in ("shortcut", "none") and x["merged"] for x in _pairs(c, m, tag)), tag
        assert all(x["lq"] == x["rlen"] and x["band"] == 3 for x in _pairs(c, m, "short_w1"))
        assert all(x["lq"] + 1 == x["rlen"] and x["band"] == 4 for x in _pairs(c, m, "short_len1"))
        n_reads = [r for r, t in zip(c.reads, c.tags) if t == "n"]
        assert all((r == 4).sum() == 1 for r in n_reads)
        strands = collections.Counter(st["out"][0][0] >= len(g) for st, t in zip(m, c.tags) if t != "long")
        assert min(strands.values()) >= 40


@pytest.mark.parametrize("okw", dc.OPTS, ids=("default", "alt"))
def test_threshold_pairs(env, okw):
    g = env[0]
    c = dc.threshold_cases(g, ac.opts(**okw)[0])
    m = _model(env, c, okw)
    for where in ("first", "last", "gap"):
        for name, d in (("at", 0), ("minus", -1), ("plus", 1)):
            ps = _pairs(c, m, "%s/%s" % (where, name))
            assert all(x["variant"].startswith("reg") and x["score"] - x["need"] == d and x["merged"] == (d >= 0) for x in ps), (where, name)
            assert {x["variant"] for x in ps} == {"reg1", "reg2", "reg3", "reg4"}
        gaps = _pairs(c, m, "gap/at") + _pairs(c, m, "gap/minus") + _pairs(c, m, "gap/plus")
        assert any(x["rlen"] > x["lq"] for x in gaps) and any(x["rlen"] < x["lq"] for x in gaps)      # deletions and insertions


@pytest.mark.parametrize("okw", dc.OPTS, ids=("default", "alt"))
def test_rounding_pairs(env, okw):
    """For each pair the two evaluations of the prediction differ (dc.rounding_cases asserts it pair by pair, with fractions
    for the contracted one), the merged score lies between their thresholds, and the oracle decides as the uncontracted
    expression does: the model, which evaluates it that way, equals the oracle."""
    g = env[0]
    opt = ac.opts(**okw)[0]
    seen = collections.Counter()
    for pad, long_rows in ((0, False), (dc.PAD, False), (0, True), (dc.PAD, True)):
        c = dc.rounding_cases(g, opt, pad, long_rows)
        m = _model(env, c, okw)
        for r, (tag, st) in enumerate(zip(c.tags, m)):
            x, = st["cands"]
            a, b = dc.pair_regs(c, r)
            un, fu = max(dc.predicted(a, b)), max(dc.predicted_fused(a, b))
            assert abs(un - fu) == 1 and x["need"] == dc.need_of(un)
            assert dc.accepts(x["score"], un) != dc.accepts(x["score"], fu) and x["merged"] == dc.accepts(x["score"], un)
            if tag[0] == "r":
                (q_un, r_un), (q_fu, r_fu) = dc.predicted(a, b), dc.predicted_fused(a, b)
                assert q_un == q_fu and r_un != r_fu and max(r_un, r_fu) > q_un      # the reference side alone tells them apart
            assert x["variant"] == ("hbm" if pad == 0 or long_rows else "lds")
            seen[tag] += 1
    assert set(seen) == {"%s%d" % (s, i) for s in "qr" for i in range(4)} and min(seen.values()) >= 8


@pytest.mark.parametrize("okw", dc.OPTS, ids=("default", "alt"))
def test_tier_reads(env, okw):
    g = env[0]
    c = dc.tier_cases(g)
    m = _model(env, c, okw)
    want = {0: "triage", 1: "triage", 2: "lane", 16: "lane", 17: "wave128", 128: "wave128", 129: "wave512", 512: "wave512", 513: "wave2048",
            2048: "wave2048", 2049: "one_lane", 2600: "one_lane"}
    it = iter(m)
    forms = [(n, form) for n in dc.TIER_SLOTS for form in (0, 1, 2)] + [(n, 0) for _ in range(dc.TIER_MORE) for n in dc.TIER_SLOTS[2:]]
    for n, form in forms:
        st = next(it)
        assert st["n_slots"] == n
        assert st["tier"] == ("triage" if form == 1 or n < 2 else want[n]), (n, form)
        if form == 2 and n >= 2:
            assert st["merges"] == 1
        if form == 0 and n >= 16:
            assert st["red"] >= 1 and st["same"] >= 1 and st["cands"]
        if st["tier"] == "one_lane":
            assert len(st["cands"]) <= 50 and all(x["lq"] <= 300 for x in st["cands"])
    per = collections.Counter(st["tier"] for st in m)
    assert all(per[t] == 10 for t in ("lane", "wave128", "wave512", "wave2048", "one_lane"))
    assert _model(env, c, okw, force_seq=True)[12]["tier"] == "one_lane"


def test_order_reads(env):
    g = env[0]
    c = dc.order_cases(g)
    for okw in dc.OPTS:
        m = _model(env, c, okw)
        by = collections.defaultdict(list)
        for t, st in zip(c.tags, m):
            by[t.split("/")[0]].append(st)
            assert st["tier"] in ("wave128", "wave512") and 65 <= st["n_slots"] <= 320, (t, st["n_slots"])
        for what in dc.ORDER_KINDS:
            assert len(by[what]) == len(dc.ORDER_LANES)
        assert all(st["merges"] == 1 and st["red"] == 0 for w in ("merge", "merge_end", "merge_rid", "interleaved") for st in by[w])
        assert all(st["merges"] == 0 and st["red"] == 1 for st in by["p_loses"])
        assert all(st["merges"] == 1 and st["red"] == 1 for st in by["q_loses"])
        assert all(st["merges"] == 2 and len(st["cands"]) == 2 for st in by["cascade"])
        assert all(st["merges"] == 0 and not st["cands"] for w in ("cross", "lpac") for st in by[w])
        assert all(len(by[w]) == 8 for w in ("interleaved", "cross", "lpac"))
    enc, cum, regs, off = c.flat()
    assert (regs["rid"] == -1).sum() >= 300 and (regs["rid"] == 1).sum() >= 300 and (regs["rb"] >= len(g)).sum() >= 1000
    assert int(np.diff(cum).max()) <= dc.EH_LDS_LEN


def test_fuzz_reaches_every_tier(env):
    """Over the eight seeds every tier meets at least 20 merges, 20 redundant drops and 20 identical-hit drops."""
    g = env[0]
    per = collections.defaultdict(collections.Counter)
    for seed in range(8):
        c = dc.fuzz_cases(g, seed)
        m = _model(env, c, {})
        for st in m:
            for k in ("merges", "red", "same"):
                per[st["tier"]][k] += st[k]
            if st["tier"] == "one_lane":
                assert len(st["cands"]) <= 50 and all(x["lq"] <= 300 for x in st["cands"])
        tiers = collections.Counter(st["tier"] for st in m)
        assert min(tiers[t] for t in ("triage", "lane", "wave128", "wave512", "wave2048", "one_lane")) >= 8, (seed, tiers)
    for tier in ("lane", "wave128", "wave512", "wave2048", "one_lane"):
        assert min(per[tier][k] for k in ("merges", "red", "same")) >= 20, (tier, per[tier])
