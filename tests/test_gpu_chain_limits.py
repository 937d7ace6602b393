"""Chaining at its limits: the planted cases of tests/chain_cases.py through bwams_chain_run_ert, with 64 seeds per pass
(BWAMS_CHAIN_BATCH=1) and one seed at a time (=0), against loader.chain_new_ert bit for bit — every field of chains, seeds and
chain_off, frac_rep included — and bwams_debug_chain_counts against the route model: the ten class counts, the many-chain and
redo lists, the wave filter's size histogram and, under BWAMS_CHAIN_COUNT=1, the in-wave and one-lane filter routes are EQUAL
to what the model derives from the inputs and the oracle's unfiltered chains, not merely positive.  tests/test_chain_cases.py
proves under the oracle alone that every case sits where it was aimed."""
import numpy as np
import pytest

import chain_cases as cc
from bwams import capi
from oracle import loader

pytestmark = pytest.mark.gpu

CHAIN_FIELDS = ("seqid", "n", "m", "first", "rid", "w_kept_alt", "frac_rep", "pos", "seed_off")
SEED_FIELDS = ("rbeg", "qbeg", "len", "score")
REG_FIELDS = ("rb", "re", "qb", "qe", "rid", "chain", "score", "truesc", "sub", "alt_sc", "csub", "sub_n", "w",
              "seedcov", "secondary", "secondary_all", "seedlen0", "n_comp_is_alt", "frac_rep", "hash", "flg")
FINAL_FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "n_comp_is_alt")
PASS_KEYS = ("in_wave", "lane_seq", "passes", "pass_seeds", "pass_new", "one_by_one")
CASES = dict(class_limits=cc.class_limits, ordered_array=cc.ordered_array, ordered_default=cc.ordered_default, settling=cc.settling, filter_limits=cc.filter_limits,
             filter_big=cc.filter_big, stride_pick=cc.stride_pick)
CASES.update({"sequences%d" % n: (lambda n=n: cc.sequences(n)) for n in (1, 64, 65, 4096, 4097)})
CASES.update({"alt_" + w: (lambda w=w: cc.alt_tables(w)) for w in ("none", "mid", "first")})
CASES.update({"filter_" + w: (lambda w=w: cc.filter_options(w)) for w in ("extend", "floor_all", "floor_some")})


@pytest.fixture(scope="module")
def ix():
    capi.lib()
    g, idx = cc.setting()
    ix = capi.Index.from_host(idx, 0)
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def wanted():
    """The oracle's answer and the model's counts per case, computed once."""
    memo = {}

    def get(case):
        if case.name not in memo:
            memo[case.name] = (case.oracle(), cc.model(case))
        return memo[case.name]
    return get


def _knobs(monkeypatch, batch, count):
    monkeypatch.setenv("BWAMS_CHAIN_BATCH", batch)
    if count:
        monkeypatch.setenv("BWAMS_CHAIN_COUNT", "1")
    else:
        monkeypatch.delenv("BWAMS_CHAIN_COUNT", raising=False)
    capi.debug_reload()                                       # the switches are read once: say that they changed


def _run(ix, case, want):
    """The case through the library: the batch, with its chains compared to `want` and the sequence table restored."""
    _, gopt = cc.mem_opts(**case.opts)
    b = capi.Batch(ix, len(case.reads), int(case.cum[-1]))
    ix.set_contigs(case.contigs if case.contigs is not None else loader.single_contig(cc.L_PAC))
    try:
        b.seed_upload(case.enc, case.cum)
        nc, ns = b.chain_run_ert(case.mems, case.mem_off, case.hits, case.hit_off, gopt)
        ch, sd, off = b.chain_fetch()
        wch, wsd, woff = want
        assert np.array_equal(off, woff) and nc == len(wch) and ns == len(wsd)
        for f in CHAIN_FIELDS:
            assert np.array_equal(ch[f], wch[f]), (case.name, f)
        for f in SEED_FIELDS:
            assert np.array_equal(sd[f], wsd[f]), (case.name, f)
    except BaseException:
        b.close()
        ix.set_contigs(loader.single_contig(cc.L_PAC))
        raise
    return b


def _check_counts(case, cnt, model, counted):
    for k in cc.COUNT_KEYS:
        if k in PASS_KEYS and not counted:
            assert cnt[k] == -1, (case.name, k)
        else:
            assert cnt[k] == model[k], (case.name, k, cnt, {x: model[x] for x in cc.COUNT_KEYS})
    if counted:
        assert cnt["pass_new"] <= cnt["pass_seeds"] and min(cnt[k] for k in PASS_KEYS) >= 0
    else:
        assert all(cnt[k] == -1 for k in PASS_KEYS)


@pytest.mark.parametrize("batch", ["1", "0"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_planted_case(ix, wanted, monkeypatch, name, batch):
    case = CASES[name]()
    want, model = wanted(case)
    _knobs(monkeypatch, batch, True)
    b = _run(ix, case, want)
    try:
        cnt = b.debug_chain_counts()
        _check_counts(case, cnt, model, True)
        assert b.stats().n_chain_redo == model["redo"]
        if batch == "0":
            assert cnt["passes"] == cnt["pass_seeds"] == cnt["pass_new"] == cnt["one_by_one"] == 0
    finally:
        b.close()
        ix.set_contigs(loader.single_contig(cc.L_PAC))


@pytest.mark.parametrize("name", ["class_limits", "ordered_array", "settling", "sequences4097", "alt_mid", "filter_limits", "filter_big", "stride_pick"])
def test_without_the_count_variable(ix, wanted, monkeypatch, name):
    """A run without BWAMS_CHAIN_COUNT launches the kernel instances that hold no counting code: the same chains, the
    unconditional counts, and -1 for what only the counting instances know."""
    case = CASES[name]()
    want, model = wanted(case)
    _knobs(monkeypatch, "1", False)
    b = _run(ix, case, want)
    try:
        _check_counts(case, b.debug_chain_counts(), model, False)
    finally:
        b.close()
        ix.set_contigs(loader.single_contig(cc.L_PAC))


def test_pass_counters_of_the_settling_reads(ix, monkeypatch):
    """Seeds at independent loci settle in passes of 64 alone; a tandem read (every hit extends the chain of the hit before)
    falls back to one seed at a time and returns to passes for its second MEM."""
    c = cc.settling()
    _knobs(monkeypatch, "1", True)
    seen = {}
    for note in ("independent", "tandem", "touched", "equal_in_pass"):
        r = c.read(note)
        one = cc.Case(note, [c.reads[r]], [note], c.opts)
        b = _run(ix, one, one.oracle())
        try:
            seen[note] = b.debug_chain_counts()
        finally:
            b.close()
    ind, tan, tou, eq = (seen[n] for n in ("independent", "tandem", "touched", "equal_in_pass"))
    assert ind["one_by_one"] == 0 and ind["passes"] == 5 and ind["pass_seeds"] == ind["pass_new"] == 300        # 4 x 64 + 44
    # the tandem MEM: a pass settles one seed (the next one must see it), then eight go one by one, per 64 seeds afresh: over 150
    # of its 200.  The second MEM's 100 loci settle in passes again, but for the at most eight that fall into a one-by-one window.
    assert tan["one_by_one"] > 150 and tan["pass_seeds"] + tan["one_by_one"] == 300
    assert tan["pass_new"] >= 1 + 100 - 8 and tan["pass_seeds"] >= 100 - 8 + 200 // 9
    # four MEMs over 20 loci: a pass ends before the first seed whose chain a seed of the same pass started or extended
    assert (tou["passes"], tou["pass_seeds"], tou["pass_new"], tou["one_by_one"]) == (5, 80, 20, 0)            # 20 + 20 + 20 + 4, then 16
    assert eq["redo"] == 1 and eq["passes"] == eq["pass_seeds"] == 0 and eq["n_heavy"] == 1 and eq["lane_seq"] == 0    # given up inside its only pass


def test_sequential_form_is_counted_apart(ix, monkeypatch):
    """3840 chains are the last that chain_heavy_kernel's largest class sorts and filters as a wave; 3841 go to one lane, and the
    device says so in a count of its own (the histogram's last bin would hold either read)."""
    big = cc.filter_big()
    _knobs(monkeypatch, "1", False)
    for note, seq in (("redo3840", 0), ("redo3841", 1)):
        one = _sub(big, [note])
        b = _run(ix, one, one.oracle())
        try:
            cnt = b.debug_chain_counts()
        finally:
            b.close()
        assert (cnt["flt_seq"], cnt["flt_more"], cnt["n_heavy"], cnt["redo"]) == (seq, 1 - seq, 1, 1), (note, cnt)


def _sub(case, notes):
    rs = [case.read(n) for n in notes]
    return cc.Case(case.name + "_sub", [case.reads[r] for r in rs], list(notes), case.opts, case.contigs, [case.lens[r] for r in rs])


CONSUMERS = dict(
    class_limits=lambda: _sub(cc.class_limits(), ["seeds32", "seeds33", "seeds128", "seeds129", "seeds257", "over_by_skipped", "all_skipped"]),
    ordered_array=lambda: _sub(cc.ordered_array(), ["chains64", "chains65", "interleave"]),
    settling=cc.settling, sequences65=lambda: cc.sequences(65),
    filter_limits=lambda: _sub(cc.filter_limits(), ["lane16", "lane17", "redo17", "redo65", "tie_blocks"]),
    filter_extend=lambda: cc.filter_options("extend"), stride_pick=cc.stride_pick, alt_mid=lambda: cc.alt_tables("mid"))


@pytest.mark.parametrize("name", sorted(CONSUMERS))
def test_consumers_take_the_chains(ix, monkeypatch, name):
    """One case per family on through extension and de-duplication: the emitted seed order is what the consumers expect."""
    case = CONSUMERS[name]()
    _knobs(monkeypatch, "1", True)
    g, _ = cc.setting()
    ref = np.concatenate([g, (3 - g[::-1]).astype(np.uint8)])
    oopt, gopt = cc.mem_opts(**case.opts)
    want = case.oracle()
    b = _run(ix, case, want)
    try:
        _consume(b, case, want, ref, oopt, gopt)
    finally:
        b.close()
        ix.set_contigs(loader.single_contig(cc.L_PAC))


def _consume(b, case, want, ref, oopt, gopt):
    b.extend_run(gopt)
    regs, reg_off, aln = b.extend_fetch()
    wregs, wreg_off, wseeds = loader.chain2aln(want[0], want[1], want[2], case.enc, case.cum, ref, cc.L_PAC, contigs=case.contigs, opt=oopt)
    assert np.array_equal(reg_off, wreg_off) and np.array_equal(aln, wseeds["aln"])
    purged = (wregs["qb"] == -1) & (wregs["qe"] == -1)
    assert np.array_equal((regs["qb"] == -1) & (regs["qe"] == -1), purged)
    for f in REG_FIELDS:
        assert np.array_equal(regs[f][~purged], wregs[f][~purged]), f
    n_fin = b.dedup_run(gopt)
    fin, fin_off = b.dedup_fetch()
    wfin, wfin_off = loader.regs_finish(wregs, wreg_off, case.enc, case.cum, ref, cc.L_PAC, contigs=case.contigs, opt=oopt)
    assert n_fin == len(wfin) and np.array_equal(fin_off, wfin_off)
    for f in FINAL_FIELDS:
        assert np.array_equal(fin[f], wfin[f]), f


def test_query_coordinates_at_the_16_bit_limit(ix, wanted, monkeypatch):
    """A read of 32768 bases is one beyond the 16-bit query fields of the chain records: BWAMS_ERR_UNSUPPORTED, and the hook has
    nothing to report, also when a good run came before the refused one.  A read of 32767 bases with seeds that end at its last
    base is chained (and, long as it is, re-scored by mem_flt_chained_seeds) like any other.  No consumer run here: extension's
    banded SW takes queries of up to 18196 bases.  One batch for all, the longer read first: a batch's seeding scratch grows
    with its longest read, which at these lengths takes seconds."""
    c = cc.coordinates()
    too_long = cc.Case("too_long", c.reads, c.notes, c.opts, None, [32768])
    _knobs(monkeypatch, "1", True)
    b = capi.Batch(ix, 1, 32768)
    try:
        b.seed_upload(too_long.enc, too_long.cum)
        with pytest.raises(capi.BwamsError) as e:
            b.chain_run_ert(too_long.mems, too_long.mem_off, too_long.hits, too_long.hit_off)
        assert e.value.code == -6                             # BWAMS_ERR_UNSUPPORTED
        with pytest.raises(capi.BwamsError):
            b.debug_chain_counts()
        want, model = wanted(c)
        b.seed_upload(c.enc, c.cum)
        nc, ns = b.chain_run_ert(c.mems, c.mem_off, c.hits, c.hit_off)
        ch, sd, off = b.chain_fetch()
        assert np.array_equal(off, want[2]) and nc == len(want[0]) and ns == len(want[1])
        for f in CHAIN_FIELDS:
            assert np.array_equal(ch[f], want[0][f]), f
        for f in SEED_FIELDS:
            assert np.array_equal(sd[f], want[1][f]), f
        assert (sd["qbeg"] + sd["len"]).max() == 32767
        _check_counts(c, b.debug_chain_counts(), model, True)
        b.seed_upload(too_long.enc, too_long.cum)             # ... and the hook reports the LAST run: a refused one has nothing
        with pytest.raises(capi.BwamsError):
            b.chain_run_ert(too_long.mems, too_long.mem_off, too_long.hits, too_long.hit_off)
        with pytest.raises(capi.BwamsError):
            b.debug_chain_counts()
    finally:
        b.close()
