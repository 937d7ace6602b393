"""bwams_dedup_run on hand-made regions (bwams_debug_ext_regs_upload), at the limits of each of its paths: the triage kernel, the
lane tier, the three instances of the wave tier and the one-lane form beyond its LDS budget; the four statements of the patch
alignment at the query lengths where one hands over to the next; the acceptance threshold and the early exit of the register
form; the rounding of mem_patch_reg's predicted scores; the order of events in the wave tier's pairwise pass.  Every field of
every final region and reg_off equal loader.regs_finish on the same regions and reads (integers: no tolerance), under the
default options and under ALT, and again under BWAMS_DEDUP_SEQ=1.  The device's own counts (bwams_debug_dedup_counts) equal
what tests/dedup_cases.py computes from the kernels' rules; a test that aims at a route asserts at least 8 items on it.
tests/test_dedup_cases.py holds the generators and the model against the oracle without a GPU."""
import collections

import numpy as np
import pytest

import aln_cases as ac
import dedup_cases as dc
from bwams import capi
from oracle import loader
from util import toy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    g, idx = toy()
    ix = capi.Index.from_host(idx, 0)
    ix.set_contigs(dc.contigs_of(len(g)))
    yield g, idx, ix
    ix.close()


@pytest.fixture(autouse=True)
def _counting(monkeypatch):
    monkeypatch.setenv("BWAMS_DEDUP_COUNT", "1")
    capi.debug_reload()                                       # the switches are read once: say that it changed


def _dedup(b, gopt, flat):
    enc, cum, regs, off = flat
    b.seed_upload(enc if len(enc) else np.zeros(1, np.uint8), cum)
    b.debug_ext_regs_upload(regs, off)
    n = b.dedup_run(gopt)
    got, goff = b.dedup_fetch()
    assert n == len(got)
    return got, goff, b.debug_dedup_counts()


def _equal(got, goff, want, woff, what=""):
    assert np.array_equal(goff, woff), what
    for f in loader.ALNREG_DTYPE.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (what, f, bad[:5], got[f][bad[:5]], want[f][bad[:5]])


def _run(dev, c, okw, monkeypatch, batch=None, seq=True):
    """Upload the reads and slots of c, run de-duplication, compare with the oracle and the device's counts with the model's;
    then the same under BWAMS_DEDUP_SEQ=1.  Returns (model per read, device counts)."""
    g, idx, ix = dev
    oopt, gopt = ac.opts(**okw)
    flat = c.flat()
    enc, cum, regs, off = flat
    contigs = dc.contigs_of(len(g))
    b = batch or capi.Batch(ix, max(len(cum) - 1, 1), max(int(cum[-1]), 1))
    got, goff, cnt = _dedup(b, gopt, flat)
    want, woff = loader.regs_finish(regs, off, enc, cum, idx.ref_0123, len(g), contigs=contigs, opt=oopt)
    m = dc.model(oopt, regs, off, enc, cum, idx.ref_0123, len(g), contigs)
    print("reads", len(cum) - 1, "slots", len(regs), "final", len(want), "device", cnt, "model", dc.counts(m))
    _equal(got, goff, want, woff)
    assert {k: cnt[k] for k in dc.COUNT_KEYS} == dc.counts(m)
    assert cnt["early"] <= sum(not x["merged"] for st in m for x in st["cands"])
    if seq:
        monkeypatch.setenv("BWAMS_DEDUP_SEQ", "1")
        capi.debug_reload()
        got2, goff2, cnt2 = _dedup(b, gopt, flat)
        monkeypatch.delenv("BWAMS_DEDUP_SEQ")
        capi.debug_reload()
        _equal(got2, goff2, want, woff, "BWAMS_DEDUP_SEQ=1")
        assert {k: cnt2[k] for k in dc.COUNT_KEYS} == dc.counts(m, force_seq=True) and cnt2["early"] == 0
        assert cnt2["one_lane"] == sum(cnt[k] for k in ("wave128", "wave512", "wave2048", "one_lane"))
        assert cnt2["wave128"] == cnt2["wave512"] == cnt2["wave2048"] == cnt2["lds"] == cnt2["reg1"] == cnt2["reg4"] == 0
    if batch is None:
        b.close()
    return m, cnt


@pytest.mark.parametrize("okw", dc.OPTS, ids=("default", "alt"))
def test_tier_edges(dev, okw, monkeypatch):
    """Reads of 0, 1, 2, 16 | 17, 128 | 129, 512 | 513, 2048 | 2049 and 2600 slots, all live, all but one and all but two purged,
    and three more all-live reads of each count: ten reads on each tier."""
    m, cnt = _run(dev, dc.tier_cases(dev[0]), okw, monkeypatch)
    assert cnt["triage"] == 16 and all(cnt[k] == 4 + 2 * dc.TIER_MORE >= 8 for k in ("lane", "wave128", "wave512", "wave2048", "one_lane"))
    assert sum(st["merges"] for st in m) >= 20 and sum(st["red"] for st in m) >= 100 and sum(st["same"] for st in m) >= 20


@pytest.mark.parametrize("setting", ("lane", "wave", "wave_hbm"))
@pytest.mark.parametrize("okw", dc.OPTS, ids=("default", "alt"))
def test_alignment_variants(dev, okw, setting, monkeypatch):
    """One patchable pair per read with l_query at 63 | 64, 127 | 128, 191 | 192, 255 | 256 and 999, both strands, an insertion,
    a deletion or a mismatch block between the halves, the gap-free shortcut and each of its conditions off by one, the band at
    dl + 3 and capped by 4 opt.w, an N in the read: alone (lane tier, row in global memory), among 17 more slots (wave tier:
    registers by NC, or LDS), and in a batch with a 1001-base read (wave tier, one lane, row in global memory)."""
    c = dc.variant_cases(dev[0], ac.opts(**okw)[0], 0 if setting == "lane" else dc.PAD, setting == "wave_hbm")
    m, cnt = _run(dev, c, okw, monkeypatch)
    assert sum(st["merges"] for st in m) == 112 and cnt["shortcut"] >= 16
    if setting == "wave":
        assert cnt["wave128"] == 112 and min(cnt[k] for k in ("reg1", "reg2", "reg3", "reg4", "lds")) >= 14 and cnt["hbm"] == 0
        assert cnt["early"] == 0                              # every pair merges: the early exit must not fire
    else:
        assert cnt["hbm"] >= 96 and cnt["lane" if setting == "lane" else "wave128"] == 112


@pytest.mark.parametrize("okw", dc.OPTS, ids=("default", "alt"))
def test_threshold_and_early_exit(dev, okw, monkeypatch):
    """Merged scores at the smallest score the acceptance test takes, one below and one above, through the register form: the
    damage in the first quarter of the rows (the early exit's bound is tightest: the pairs at and above the threshold must come
    through, those one below are ended early), in the last quarter, or one gap followed by perfect matches."""
    g = dev[0]
    c = dc.threshold_cases(g, ac.opts(**okw)[0])
    merged, first_minus, other_minus = (dc.Cases(g) for _ in range(3))
    for r, t in enumerate(c.tags):
        dst = merged if not t.endswith("minus") else first_minus if t.startswith("first") else other_minus
        dst.reads.append(c.reads[r]); dst.slots.append(c.slots[r]); dst.tags.append(t)
    m, cnt = _run(dev, merged, okw, monkeypatch)
    assert all(st["merges"] == 1 for st in m) and len(m) == 60
    assert cnt["early"] == 0 and sum(cnt[k] for k in ("reg1", "reg2", "reg3", "reg4")) == 60
    m, cnt = _run(dev, first_minus, okw, monkeypatch)
    assert all(st["merges"] == 0 for st in m) and len(m) == 10
    assert cnt["early"] >= 8, cnt                             # a bad first quarter, then matches only: the bound says so at once
    m, cnt = _run(dev, other_minus, okw, monkeypatch)
    assert all(st["merges"] == 0 for st in m) and len(m) == 20


@pytest.mark.parametrize("setting", ("lane", "wave", "wave_hbm"))
@pytest.mark.parametrize("okw", dc.OPTS, ids=("default", "alt"))
def test_rounding_edge(dev, okw, setting, monkeypatch):
    """mem_patch_reg's predicted scores where ratio * score sum + .499 is an integer: contracted into one fused multiply-add the
    prediction is one off, and the merged score of these pairs is the one at which the acceptance test tells the two apart.
    Through the lane tier, the wave tier's LDS form, and (the rows whose merged query span exceeds 1000 bases) its one-lane form."""
    c = dc.rounding_cases(dev[0], ac.opts(**okw)[0], 0 if setting == "lane" else dc.PAD, setting == "wave_hbm")
    if setting == "lane":
        c.extend(dc.rounding_cases(dev[0], ac.opts(**okw)[0], 0, True))
    m, cnt = _run(dev, c, okw, monkeypatch)
    assert cnt["lds" if setting == "wave" else "hbm"] >= 24
    assert len({st["merges"] for st in m}) == (2 if setting != "wave_hbm" else 1)      # both directions of the flip occur


def test_wave_tier_event_order(dev, monkeypatch):
    """Scans of two to five chunks of 64 upstream regions: merges, cascades (the regions further upstream are tested again
    after a merge), redundant pairs with either loser, each on the first and on the last lane of a chunk, a merge that ends the
    scan, two sequences interleaved by end, a pair across the strands, a region that spans l_pac, rid -1, the ALT sequence."""
    c = dc.order_cases(dev[0])
    for okw in dc.OPTS:
        m, cnt = _run(dev, c, okw, monkeypatch)
        assert cnt["wave128"] >= 8 and cnt["wave512"] >= 8 and cnt["lds"] + cnt["reg3"] + cnt["reg4"] >= 60
        kinds = collections.Counter((t.split("/")[0], st["merges"], st["red"]) for t, st in zip(c.tags, m))
        assert kinds[("cascade", 2, 0)] == kinds[("q_loses", 1, 1)] == kinds[("p_loses", 0, 1)] == len(dc.ORDER_LANES)


@pytest.mark.parametrize("seed", range(8))
def test_fuzz(dev, seed, monkeypatch):
    """Some 210 reads whose slot counts are drawn across all tiers, under both option sets."""
    c = dc.fuzz_cases(dev[0], seed)
    for okw in dc.OPTS:
        m, cnt = _run(dev, c, okw, monkeypatch)
        assert min(cnt[k] for k in ("triage", "lane", "wave128", "wave512", "wave2048", "one_lane")) >= 8


def test_reuse_and_empty_batches(dev, monkeypatch):
    """A small batch, a large one and the small one again on one Batch: the buffers grow, the counters start from zero, the
    two small runs are equal.  Then a batch without reads and one in which no read has a slot."""
    g, idx, ix = dev
    small, large = dc.variant_cases(g, ac.opts()[0], dc.PAD), dc.fuzz_cases(g, 3)
    nb = max(int(x.flat()[1][-1]) for x in (small, large))
    b = capi.Batch(ix, 256, nb)
    _, c1 = _run(dev, small, {}, monkeypatch, batch=b, seq=False)
    first = b.dedup_fetch()
    _, c2 = _run(dev, large, {}, monkeypatch, batch=b, seq=False)
    _, c3 = _run(dev, small, {}, monkeypatch, batch=b, seq=False)
    again = b.dedup_fetch()
    assert c1 == c3 and c1 != c2
    _equal(again[0], again[1], first[0], first[1])
    empty = dc.Cases(g)
    m, cnt = _run(dev, empty, {}, monkeypatch, batch=b)
    assert m == [] and not any(cnt.values())
    for r in small.reads[:40]:
        empty.read(r, "bare")
    m, cnt = _run(dev, empty, {}, monkeypatch, batch=b)
    assert cnt["triage"] == 40 and sum(cnt.values()) == 40
    b.close()


def test_counts_need_the_switch(dev, monkeypatch):
    """Without BWAMS_DEDUP_COUNT the kernels get no counters, and the hook says that nothing was counted."""
    g, idx, ix = dev
    monkeypatch.delenv("BWAMS_DEDUP_COUNT")
    capi.debug_reload()
    flat = dc.variant_cases(g, ac.opts()[0], dc.PAD).flat()
    b = capi.Batch(ix, len(flat[1]) - 1, int(flat[1][-1]))
    b.seed_upload(flat[0], flat[1])
    b.debug_ext_regs_upload(flat[2], flat[3])
    b.dedup_run(ac.opts()[1])
    with pytest.raises(capi.BwamsError) as e:
        b.debug_dedup_counts()
    assert e.value.code == -3
    b.close()


def test_hook_arguments(dev):
    """bwams_debug_ext_regs_upload refuses what would make a kernel read outside the reads or the text and what the reference
    itself divides by zero on, with BWAMS_ERR_ARG, and leaves the batch's earlier final regions fetchable and unchanged."""
    g, idx, ix = dev
    oopt, gopt = ac.opts()
    enc, cum, regs, off = dc.variant_cases(g, oopt, 3).flat()
    b = capi.Batch(ix, len(cum) - 1, int(cum[-1]))
    b.seed_upload(enc, cum)
    with pytest.raises(capi.BwamsError):                      # nothing to run on yet
        b.dedup_run(gopt)
    b.debug_ext_regs_upload(regs, off)
    b.dedup_run(gopt)
    fin = b.dedup_fetch()

    def refused(r, o):
        with pytest.raises(capi.BwamsError) as e:
            b.debug_ext_regs_upload(r, o)
        assert e.value.code == -3
        now = b.dedup_fetch()
        _equal(now[0], now[1], fin[0], fin[1])

    refused(regs, off[:-1])                                    # not the uploaded read count
    o = off.copy(); o[0] = 1
    refused(regs, o)
    refused(regs[:-1], off)                                    # reg_off does not end at n_regs
    o = off.copy(); o[3], o[4] = off[4], off[3]
    refused(regs, o)                                           # decreasing
    k = int(off[5])                                            # a live region of read 5
    assert regs["qe"][k] > regs["qb"][k]
    l_pac = len(g)
    for f, v in (("qb", -1), ("qe", int(cum[6] - cum[5]) + 1), ("rb", -1), ("re", 2 * l_pac + 1), ("re", int(regs["rb"][k])),
                 ("score", 0), ("rid", 3), ("rid", -2)):
        r = regs.copy(); r[f][k] = v
        refused(r, off)
    r = regs.copy(); r["qb"][k] = r["qe"][k] = -1; r["rid"][k] = 7     # a purged slot keeps its freedom, but not its rid
    refused(r, off)
    for qb, qe in ((-1, -1), (9, 9), (9, 3)):                  # purged slots pass as they are
        r = regs.copy(); r["qb"][k], r["qe"][k], r["rb"][k], r["re"][k], r["score"][k] = qb, qe, -5, -9, 0
        b.debug_ext_regs_upload(r, off)
        with pytest.raises(capi.BwamsError):                  # everything downstream counts as outdated
            b.dedup_fetch()
        b.dedup_run(gopt)
        got = b.dedup_fetch()
        want = loader.regs_finish(r, off, enc, cum, idx.ref_0123, l_pac, contigs=dc.contigs_of(l_pac), opt=oopt)
        _equal(got[0], got[1], want[0], want[1])
    b.close()
