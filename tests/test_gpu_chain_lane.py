"""The lane tier of the chaining stage (csrc/chain_lane.hip): the planted reads of tests/chain_lane_cases.py through
bwams_chain_run_ert against loader.chain_new_ert bit for bit — every field of chains, seeds and chain_off — with the kernel
instance a production run launches and with the counting one, and bwams_debug_chain_lane_counts EQUAL to the model: the reads
of at most 32 seeds, and those among them the oracle gives more than nine chains before the filter (they give the leaf form
up and are chained again through the B-tree).  tests/test_chain_lane_cases.py proves under the oracle alone that every case has
the property it is built for."""
import numpy as np
import pytest

import chain_cases as cc
import chain_lane_cases as lc
from bwams import capi
from oracle import loader

pytestmark = pytest.mark.gpu

CHAIN_FIELDS = ("seqid", "n", "m", "first", "rid", "w_kept_alt", "frac_rep", "pos", "seed_off")
SEED_FIELDS = ("rbeg", "qbeg", "len", "score")


@pytest.fixture(scope="module")
def ix():
    capi.lib()
    g, idx = cc.setting()
    ix = capi.Index.from_host(idx, 0)
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def wanted():
    """The oracle's answer and the lane model per case, computed once."""
    memo = {}

    def get(case):
        if case.name not in memo:
            memo[case.name] = (case.oracle(), lc.lane_model(case))
        return memo[case.name]
    return get


def _knobs(monkeypatch, count):
    if count:
        monkeypatch.setenv("BWAMS_CHAIN_COUNT", "1")
    else:
        monkeypatch.delenv("BWAMS_CHAIN_COUNT", raising=False)
    capi.debug_reload()                                       # the switches are read once: say that they changed


def _run(ix, case, want):
    """The case through the library, field for field against `want`; -> (lane-tier reads, give-ups, route counts)."""
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
        return b.debug_chain_lane_counts(), b.debug_chain_counts()
    finally:
        b.close()
        ix.set_contigs(loader.single_contig(cc.L_PAC))


@pytest.mark.parametrize("count", [False, True], ids=["plain", "counting"])
@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_planted_case(ix, wanted, monkeypatch, name, count):
    case = lc.CASES[name]()
    want, model = wanted(case)
    _knobs(monkeypatch, count)
    lane, cnt = _run(ix, case, want)
    assert lane == model, (name, lane, model)
    if count:                                                 # every lane-tier read with a chain is sorted and filtered by its lane
        routes = cc.model(case)
        assert cnt["lane_seq"] == routes["lane_seq"] and cnt["gt_lane"] == routes["gt_lane"], (name, cnt)


@pytest.mark.parametrize("note,gave_up", [("nine_of_10", 0), ("ten_of_10", 1), ("nine_of_32", 0), ("ten_of_32", 1)])
def test_give_up_count_of_the_full_leaf(ix, monkeypatch, note, gave_up):
    """Nine chains fill the leaf and stay in it; the tenth makes the read give up — after one seed each (10 seeds) or after
    three rows of a ladder have linked 27 seeds into the nine (32 seeds).  The read alone in its batch."""
    case = lc.one(lc.leaf_full(), note)
    _knobs(monkeypatch, False)
    lane, _ = _run(ix, case, case.oracle())
    assert lane == (1, gave_up)
