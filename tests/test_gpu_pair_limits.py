"""bwams_pair_run on hand-made regions (bwams_debug_pair_regs_upload), at the limits of each of its paths: mate rescue by one
lane, by a wavefront with the list in LDS and by one lane beyond its LDS capacity, the ERT variant, the rank sort, the bitonic
network and the introsort that equal keys hand over to, the insertion point and the chunked shift, the second pass;
mem_mark_primary_se by one lane, by either wave instance and beyond them, in the single-end form and as ends of pairs;
mem_reorder_primary5 and mem_pair on long lists.  Every field of every region, reg_off and every field of the pair records equal
loader.pair_pe / loader.mark_primary_se on the same input (integers: no tolerance).  The device's own counts
(bwams_debug_pair_counts) equal what tests/pair_cases.py computes from the kernels' rules; a test that aims at a route asserts
at least 8 reads on it.  tests/test_pair_cases.py holds the generators against the oracle without a GPU."""
import collections

import numpy as np
import pytest

import aln_cases as ac
import pair_cases as pc
from bwams import capi
from oracle import loader

pytestmark = pytest.mark.gpu

MODEL_KEYS = pc.ROUTE_KEYS + ("post_second",)


@pytest.fixture(scope="module")
def dev():
    g, idx = pc.setting()
    ix = capi.Index.from_host(idx, 0)
    yield g, idx, ix
    ix.close()


@pytest.fixture(autouse=True)
def _counting(monkeypatch):
    monkeypatch.setenv("BWAMS_PAIR_COUNT", "1")
    capi.debug_reload()                                       # the switches are read once: say that it changed


def _equal(got, goff, want, woff, what=""):
    assert np.array_equal(goff, woff), what
    for f in pc.REG_FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (what, f, bad[:5], got[f][bad[:5]], want[f][bad[:5]])


def _batch(ix, flat):
    enc, cum, regs, off = flat
    return capi.Batch(ix, max(len(cum) - 1, 2), max(int(cum[-1]), 1))


def _upload(b, ix, c, flat):
    enc, cum, regs, off = flat
    ix.set_contigs(c.contigs)
    b.seed_upload(enc if len(enc) else np.zeros(1, np.uint8), cum)
    b.debug_pair_regs_upload(regs, off)


def _run(dev, c, pes, use_ert=False, no_rescue=False, sflag=0, T=30, id_base=0, batch=None, drop_plan=False, what=""):
    """Upload the reads and regions of c, run the paired-end tail, compare regions, offsets and pair records with the oracle,
    the run's statistics with the model's plan and the device's counts with the model's routes.  Returns (counts, oracle result)."""
    g, idx, ix = dev
    oopt, gopt = ac.opts()
    flat = c.flat()
    enc, cum, regs, off = flat
    b = batch or _batch(ix, flat)
    _upload(b, ix, c, flat)
    sopt = None
    if sflag:
        sopt = capi.default_sam_opt(sflag)
        sopt.T = T
    n, n_tasks = b.pair_run(pes, gopt, id_base=id_base, no_rescue=no_rescue, use_ert=use_ert, sopt=sopt)
    got, goff, gpairs = b.pair_fetch()
    cnt, st = b.debug_pair_counts(), b.stats()
    no_resc = no_rescue or bool(sflag & 0x20)
    want, woff, wpairs = loader.pair_pe(regs, off, enc, cum, idx.ref_0123, pc.L_PAC, pes, contigs=c.contigs, opt=oopt, id_base=id_base,
                                        no_rescue=no_resc, use_ert=use_ert, no_pairing=bool(sflag & 0x4), primary5_T=T if sflag & 0x800 else -1)
    print(what, "reads", len(cum) - 1, "regions", len(regs), "->", len(want), "tasks", n_tasks, "redone", st.n_pair_redone, cnt)
    _equal(got, goff, want, woff, what)
    for f in pc.PAIR_FIELDS:
        assert np.array_equal(gpairs[f], wpairs[f]), (what, f)
    assert n == len(want) == st.n_pair_regs and n_tasks == st.n_pair_tasks
    plan = [[] for _ in range(len(cum) - 1)] if no_resc else pc.planned(oopt, c.contigs, pes, regs, off, cum)
    redone = set()
    if drop_plan:                                             # nothing planned first: every read that wants a window is redone, every orientation
        redone = {r for r, ws in enumerate(plan) if ws}
        every = pc.planned(oopt, c.contigs, pes, regs, off, cum, every=True)
        assert st.n_pair_redone == len(redone) and n_tasks == sum(len(every[r]) for r in redone), what
    else:                                                     # no dropped region was consistent with an anchor: nobody needs the second pass
        assert st.n_pair_redone == 0 and n_tasks == sum(len(ws) for ws in plan), what
    assert {k: cnt[k] for k in MODEL_KEYS} == pc.routes(oopt, regs, off, woff, use_ert, redone, no_resc), what
    added = np.diff(woff) - np.diff(off)
    assert int(added[added > 0].sum()) <= cnt["inserted"] <= n_tasks, what
    assert cnt["sort_intro"] <= cnt["sort_rank"] + cnt["sort_net"]
    assert cnt["mark_rank"] == sum(pc.MARK_LIGHT < x <= pc.RANK_MAX for x in np.diff(woff))
    assert cnt["mark_net"] == sum(pc.RANK_MAX < x <= pc.MARK_LDS for x in np.diff(woff))
    if batch is None:
        b.close()
    return cnt, (want, woff, wpairs)


def _drop_plan(monkeypatch, on):
    if on:
        monkeypatch.setenv("BWAMS_PAIR_DROP_PLAN", "1")
    else:
        monkeypatch.delenv("BWAMS_PAIR_DROP_PLAN")
    capi.debug_reload()


@pytest.mark.parametrize("alt", (False, True), ids=("one_seq", "alt"))
def test_capacity_limits(dev, alt, monkeypatch):
    """Capacity 16 | 17 and 1024 | 1025, lists of 0 and 1 region, mates with 50 anchors, anchors that find their orientation
    consistent by then: FR only and all four orientations, the ERT variant, and every tier again through the second pass."""
    c = pc.capacity_cases(alt)
    b = _batch(dev[2], c.flat())
    cnt, _ = _run(dev, c, pc.PES_FR, batch=b, what="fr")
    assert cnt["post_lane"] >= 24 and cnt["post_wave"] >= 16 and cnt["post_one_lane"] == 8 and cnt["post_ert"] == 0
    assert cnt["inserted"] >= 8 * 6 + 8 * 3 and cnt["sort_rank"] >= 16 and cnt["sort_net"] >= 8
    cnt, _ = _run(dev, c, pc.PES_ALL, batch=b, id_base=12345, what="all four")
    assert cnt["post_lane"] >= 24 and cnt["post_one_lane"] == 8
    cnt, _ = _run(dev, c, pc.PES_FR, use_ert=True, batch=b, what="ert")
    assert cnt["post_ert"] == len(c.reads) and cnt["sort_rank"] == cnt["sort_net"] == 0 and cnt["inserted"] >= 72
    cnt, _ = _run(dev, c, pc.PES_ALL, use_ert=True, batch=b, what="ert, all four")
    _drop_plan(monkeypatch, True)
    cnt, _ = _run(dev, c, pc.PES_FR, batch=b, drop_plan=True, what="second pass")
    assert cnt["post_second"] >= 64 and cnt["post_one_lane"] == 16
    cnt, _ = _run(dev, c, pc.PES_FR, use_ert=True, batch=b, drop_plan=True, what="second pass, ert")
    assert cnt["post_second"] >= 64
    _drop_plan(monkeypatch, False)
    b.close()


@pytest.mark.parametrize("alt", (False, True), ids=("one_seq", "alt"))
def test_sort_lengths(dev, alt, monkeypatch):
    """Lists of 96 | 97 at the first sort, 127 .. 129, 512 | 513 and 1020 (the network's paddings), two rescued regions each."""
    c = pc.sort_cases(alt)
    b = _batch(dev[2], c.flat())
    cnt, _ = _run(dev, c, pc.PES_FR, batch=b, what="fr")
    n_rank, n_net = 8, 8 * 7                                   # reads built for either path, each with at least two sorts per rescue
    assert cnt["post_wave"] >= 64 and cnt["sort_rank"] >= 2 * n_rank and cnt["sort_net"] >= 2 * n_net and cnt["sort_intro"] == 0
    _run(dev, c, pc.PES_ALL, batch=b, what="all four")
    _run(dev, c, pc.PES_FR, use_ert=True, batch=b, what="ert")
    _drop_plan(monkeypatch, True)
    cnt, _ = _run(dev, c, pc.PES_FR, batch=b, drop_plan=True, what="second pass")
    assert cnt["post_second"] >= 64 and cnt["sort_net"] >= 2 * n_net
    _drop_plan(monkeypatch, False)
    b.close()


@pytest.mark.parametrize("alt", (False, True), ids=("one_seq", "alt"))
def test_insertion_points(dev, alt):
    """The rescued region in front of 64 and of 128 fillers, behind all of them, at 63 | 64 | 65 and 127 | 128, behind fillers
    of its own score: by one wavefront (the chunked shift) and, the short lists of `eq`, by one lane (capacity 14)."""
    c = pc.insertion_cases(alt)
    cnt, _ = _run(dev, c, pc.PES_FR)
    assert cnt["post_wave"] >= 80 and cnt["inserted"] >= len(c.tags)
    _run(dev, c, pc.PES_FR, use_ert=True, what="ert")


@pytest.mark.parametrize("alt", (False, True), ids=("one_seq", "alt"))
def test_equal_keys(dev, alt):
    """Fillers that share their end, in lists sorted by rank and by the network: the introsort takes over, and its order decides
    which of two mutually redundant fillers of equal score survives (tests/test_pair_cases.py: the other order gives another result)."""
    c = pc.tie_cases(alt)
    cnt, _ = _run(dev, c, pc.PES_FR)
    assert cnt["sort_intro"] >= 16 and cnt["sort_rank"] >= 8 and cnt["sort_net"] >= 8
    _run(dev, c, pc.PES_FR, use_ert=True, what="ert")
    _run(dev, pc.tie_cases(alt, swap=True), pc.PES_FR, what="swapped")


@pytest.mark.parametrize("alt", (False, True), ids=("one_seq", "alt"))
def test_dedup_effects_windows_and_mate_lengths(dev, alt):
    """A rescued region that loses to a filler and one that wins, a filler sharing its end (the ERT variant's resort), a filler
    that makes the orientation consistent; anchors at the ends of the text, of the strands and of the sequences, windows of
    min_seed_len and one less; mates of 249 | 250 and 512 bases."""
    for name in ("dedup", "window", "matelen"):
        c = pc.RESCUE_FILES[name](alt)
        cnt, (want, woff, pairs) = _run(dev, c, pc.RESCUE_PES[name], what=name)
        assert cnt["post_lane"] + cnt["post_wave"] == len(c.reads)
        cnt, _ = _run(dev, c, pc.RESCUE_PES[name], use_ert=True, id_base=9, what=name + ", ert")
        assert cnt["post_ert"] == len(c.reads)


@pytest.mark.parametrize("seed", range(4))
def test_fuzz(dev, seed, monkeypatch):
    """Some 200 reads whose list sizes are drawn around every limit, one to three anchors, all four orientations: plain, the ERT
    variant and through the second pass."""
    c = pc.fuzz_cases(bool(seed & 1), seed)
    b = _batch(dev[2], c.flat())
    cnt, _ = _run(dev, c, pc.PES_ALL, id_base=1000 * seed, batch=b, what="all four")
    assert min(cnt[k] for k in ("post_lane", "post_wave", "post_one_lane", "mark_lane", "mark_wave256", "mark_wave2048")) >= 8
    assert cnt["sort_rank"] >= 8 and cnt["sort_net"] >= 8 and cnt["sort_intro"] >= 8
    _run(dev, c, pc.PES_ALL, use_ert=True, batch=b, what="ert")
    _drop_plan(monkeypatch, True)
    _run(dev, c, pc.PES_FR, batch=b, drop_plan=True, what="second pass")
    _drop_plan(monkeypatch, False)
    b.close()


@pytest.mark.parametrize("alt", (False, True), ids=("one_seq", "alt"))
def test_marking_single_end(dev, alt):
    """mem_mark_primary_se through BWAMS_PAIR_SINGLE_END: 55 reads (odd) of 0, 1, 24 | 25, 96 | 97, 128 | 129, 256 | 257,
    2048 | 2049 and 2600 regions, all primary, mixed, all ALT and with one primary, ids from 1001 on; then with MEM_F_PRIMARY5."""
    g, idx, ix = dev
    oopt, gopt = ac.opts()
    c = pc.mark_cases(alt)
    flat = c.flat()
    enc, cum, regs, off = flat
    b = _batch(ix, flat)
    sizes = np.diff(off)
    for T in (-1, 30):
        _upload(b, ix, c, flat)
        sopt = None
        if T >= 0:
            sopt = capi.default_sam_opt(0x800)
            sopt.T = T
        n = b.mark_primary_se(gopt, id_base=1001, sopt=sopt)
        got, goff, _ = b.pair_fetch()
        assert n == len(regs) and np.array_equal(goff, off)
        want = np.concatenate([loader.mark_primary_se(regs[off[r]:off[r + 1]], 1001 + r, oopt, primary5_T=T)[0] for r in range(len(sizes))])
        _equal(got, goff, want, off, "T=%d" % T)
        cnt = b.debug_pair_counts()
        print(cnt)
        assert {k: cnt[k] for k in MODEL_KEYS} == pc.routes(oopt, regs, off, off, no_rescue=True)
        assert min(cnt[k] for k in ("mark_lane", "mark_wave256", "mark_wave2048", "mark_one_lane")) >= 8
        assert cnt["mark_rank"] == sum(pc.MARK_LIGHT < x <= pc.RANK_MAX for x in sizes) >= 8
        assert cnt["mark_net"] == sum(pc.RANK_MAX < x <= pc.MARK_LDS for x in sizes) >= 8
        assert cnt["inserted"] == cnt["sort_rank"] == cnt["sort_net"] == 0
    b.close()


@pytest.mark.parametrize("alt", (False, True), ids=("one_seq", "alt"))
def test_marking_and_mem_pair_on_long_lists(dev, alt):
    """The same reads as ends of pairs (no rescue): mem_pair over up to 2600 primaries per end, all orientations and with RF
    failed, ends without primaries, MEM_F_NOPAIRING, MEM_F_PRIMARY5, the ERT flag."""
    c = pc.mark_cases(alt)
    c.reads, c.regs, c.tags = c.reads[:54], c.regs[:54], c.tags[:27]
    b = _batch(dev[2], c.flat())
    cnt, (want, woff, pairs) = _run(dev, c, pc.PES_ALL, no_rescue=True, id_base=77, batch=b, what="all four")
    assert min(cnt[k] for k in ("mark_lane", "mark_wave256", "mark_wave2048", "mark_one_lane")) >= 8
    assert (pairs["n_pri"].min(axis=1) >= 2049).sum() >= 1 and (pairs["score"] > 0).sum() >= 8
    _run(dev, c, pc.PES_RF_FAILED, sflag=0x20, id_base=77, batch=b, what="rf failed, -S")
    cnt, (_, _, pairs) = _run(dev, c, pc.PES_ALL, sflag=0x20 | 0x4, batch=b, what="-P")
    assert (pairs["score"] == 0).all() and (pairs["z"] == -1).all()
    _run(dev, c, pc.PES_ALL, sflag=0x20 | 0x800, T=30, batch=b, what="-5")
    cnt, _ = _run(dev, c, pc.PES_ALL, no_rescue=True, use_ert=True, batch=b, what="ert flag")
    assert cnt["post_ert"] == len(c.reads)
    b.close()


def test_sam_flags_with_rescue(dev):
    """bwams_pair_run_sam on rescued lists: MEM_F_PRIMARY5, MEM_F_NOPAIRING and MEM_F_NO_RESCUE."""
    c = pc.insertion_cases(True)
    b = _batch(dev[2], c.flat())
    _run(dev, c, pc.PES_FR, sflag=0x800, T=30, batch=b, what="-5")
    _run(dev, c, pc.PES_ALL, sflag=0x800 | 0x4, T=100, id_base=5, batch=b, what="-5 -P")
    cnt, _ = _run(dev, c, pc.PES_FR, sflag=0x20, batch=b, what="-S")
    assert cnt["inserted"] == 0
    b.close()


def test_reuse_large_then_small(dev, monkeypatch):
    """Large, small, large and small again on one Batch, the second large run through the second pass: the list of long reads,
    the ticket counters and the second pass's flags start afresh, and equal inputs give equal counts and results."""
    g, idx, ix = dev
    large, small = pc.sort_cases(True), pc.dedup_cases(True)
    b = _batch(ix, large.flat())
    c1, _ = _run(dev, large, pc.PES_FR, batch=b, what="large")
    c2, _ = _run(dev, small, pc.PES_NARROW, batch=b, what="small")
    first = b.pair_fetch()
    _drop_plan(monkeypatch, True)
    c3, _ = _run(dev, large, pc.PES_FR, batch=b, drop_plan=True, what="large, second pass")
    _drop_plan(monkeypatch, False)
    c4, _ = _run(dev, small, pc.PES_NARROW, batch=b, what="small again")
    again = b.pair_fetch()
    assert c2 == c4 and c1 != c2 and c3["post_second"] > 0 == c4["post_second"]
    _equal(again[0], again[1], first[0], first[1])
    empty = pc.Cases(True)
    empty.pair(small.reads[0], [], small.reads[1], [], "bare")
    cnt, _ = _run(dev, empty, pc.PES_FR, batch=b, what="no regions")
    assert cnt["post_lane"] == cnt["mark_lane"] == 2 and sum(cnt.values()) == 4
    b.close()


def test_counts_need_the_switch(dev, monkeypatch):
    """Without BWAMS_PAIR_COUNT the kernels get no counters, and the hook says that nothing was counted."""
    g, idx, ix = dev
    monkeypatch.delenv("BWAMS_PAIR_COUNT")
    capi.debug_reload()
    c = pc.dedup_cases(False)
    flat = c.flat()
    b = _batch(ix, flat)
    _upload(b, ix, c, flat)
    with pytest.raises(capi.BwamsError) as e:                 # nothing ran yet
        b.debug_pair_counts()
    assert e.value.code == -3
    b.pair_run(pc.PES_NARROW, ac.opts()[1])
    with pytest.raises(capi.BwamsError) as e:
        b.debug_pair_counts()
    assert e.value.code == -3
    b.close()


def test_hook_arguments(dev):
    """bwams_debug_pair_regs_upload refuses what bwams_debug_regs_upload refuses and what would make a pairing kernel index outside
    the sequence table or compute on nonsense, with BWAMS_ERR_ARG, and leaves the batch as it was: the earlier result stays
    fetchable, and the same run on the same batch succeeds afterwards."""
    g, idx, ix = dev
    oopt, gopt = ac.opts()
    c = pc.dedup_cases(True)
    flat = c.flat()
    enc, cum, regs, off = flat
    b = _batch(ix, flat)
    _, (want, woff, wpairs) = _run(dev, c, pc.PES_NARROW, batch=b)
    k = int(off[1])                                            # the first region of read 1
    n_seqs = len(c.contigs)

    def refused(r, o):
        with pytest.raises(capi.BwamsError) as e:
            b.debug_pair_regs_upload(r, o)
        assert e.value.code == -3
        now = b.pair_fetch()                                   # nothing was outdated, nothing was overwritten
        _equal(now[0], now[1], want, woff)
        n, _ = b.pair_run(pc.PES_NARROW, gopt)                 # and the regions uploaded before are still the input
        got = b.pair_fetch()
        assert n == len(want)
        _equal(got[0], got[1], want, woff)

    refused(regs, off[:-1])                                    # not the uploaded read count
    o = off.copy(); o[0] = 1
    refused(regs, o)
    refused(regs[:-1], off)                                    # reg_off does not end at n_regs
    o = off.copy(); o[3], o[4] = off[4], off[3]
    refused(regs, o)                                           # decreasing
    for f, v in (("qb", -1), ("qe", int(cum[2] - cum[1]) + 1), ("rid", -1), ("rid", n_seqs), ("rb", -1), ("re", 2 * pc.L_PAC + 1),
                 ("re", int(regs["rb"][k])), ("score", -1)):
        r = regs.copy(); r[f][k] = v
        refused(r, off)
    r = regs.copy(); r["score"][k] = 0; r["re"][-1] = 2 * pc.L_PAC     # the last values the hook takes
    r["rid"][-1] = pc.rid_of(c.contigs, int(r["rb"][-1]))
    b.debug_pair_regs_upload(r, off)
    with pytest.raises(capi.BwamsError):                      # everything downstream counts as outdated
        b.pair_fetch()
    b.debug_regs_upload(regs.copy(), off)                      # the older hook keeps its contract: the reference side is not its business
    r = regs.copy(); r["rid"][k] = -1; r["re"][k] = r["rb"][k]
    b.debug_regs_upload(r, off)
    b.close()


def test_unsupported_is_refused_before_any_launch(dev):
    """Reads of 513 bases, or a window (high - low + read length) above 20000: BWAMS_ERR_UNSUPPORTED, and the earlier result of the
    batch stays as it was; without rescue the same inputs run."""
    g, idx, ix = dev
    oopt, gopt = ac.opts()
    c = pc.Cases(False)
    ref2 = idx.ref_0123
    c.pair(ref2[1000:1513], [pc.reg(c.contigs, 1000, 1513, 0, 513, 400)], ref2[30000:30150], [pc.reg(c.contigs, 30000, 30150, 0, 150, 150)], "long")
    flat = c.flat()
    b = _batch(ix, flat)
    _upload(b, ix, c, flat)
    with pytest.raises(capi.BwamsError) as e:
        b.pair_run(pc.PES_FR, gopt)
    assert e.value.code == -6
    n, n_tasks = b.pair_run(pc.PES_FR, gopt, no_rescue=True)
    assert (n, n_tasks) == (2, 0)
    first = b.pair_fetch()
    with pytest.raises(capi.BwamsError) as e:
        b.pair_run(pc.PES_FR, gopt)
    assert e.value.code == -6
    again = b.pair_fetch()
    _equal(again[0], again[1], first[0], first[1])
    b.close()
    c = pc.dedup_cases(False)
    flat = c.flat()
    b = _batch(ix, flat)
    _upload(b, ix, c, flat)
    for high, ok in ((100 + 20000 - pc.SEG, True), (100 + 20000 - pc.SEG + 1, False)):
        pes = pc.pes_of(low=100, high=high, avg=300.0, std=50.0)
        if ok:
            b.pair_run(pes, gopt)
        else:
            with pytest.raises(capi.BwamsError) as e:
                b.pair_run(pes, gopt)
            assert e.value.code == -6
    b.close()
