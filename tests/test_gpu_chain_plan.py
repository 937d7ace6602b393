"""The launch plan of the chaining stage (launch_chain_t, csrc/chain_wave.h) with every lane at work: the batch of
tests/chain_plan_cases.py — a read at both seed-count limits of every wave class, lane-tier reads between them (one that needs
a tenth chain, reads without a seed), a redo read and reads for two classes of the many-chain filter — through
bwams_chain_run_ert against loader.chain_new_ert, every field of chains, seeds and chain_off, with the kernel instances a
production run launches and with the counting ones.  bwams_debug_chain_counts' class counts are EQUAL to the counts planted,
its other counts to the route model's.  The stage runs three times on the same batch and returns the same bytes: a launch that
the join does not wait for, or a ticket that a run leaves behind, shows up in the second and third.
tests/test_chain_plan_cases.py proves under the oracle alone that the batch holds what it is built for."""
import numpy as np
import pytest

import chain_cases as cc
import chain_plan_cases as pc
from bwams import capi
from oracle import loader

pytestmark = pytest.mark.gpu

CHAIN_FIELDS = ("seqid", "n", "m", "first", "rid", "w_kept_alt", "frac_rep", "pos", "seed_off")
SEED_FIELDS = ("rbeg", "qbeg", "len", "score")
COUNTED_ONLY = ("in_wave", "lane_seq")                        # routes that only the counting instances count


@pytest.fixture(scope="module")
def ix():
    capi.lib()
    g, idx = cc.setting()
    ix = capi.Index.from_host(idx, 0)
    ix.set_contigs(loader.single_contig(cc.L_PAC))
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def wanted():
    """(case, seeds planted, the oracle's answer, the route model, the lane model): computed once, never changed."""
    case, planted = pc.plan_batch()
    return case, planted, case.oracle(), cc.model(case), pc.lc.lane_model(case)


@pytest.mark.parametrize("count", [False, True], ids=["plain", "counting"])
def test_every_lane_at_once_three_times(ix, wanted, monkeypatch, count):
    case, planted, (wch, wsd, woff), model, lane_model = wanted
    if count:
        monkeypatch.setenv("BWAMS_CHAIN_COUNT", "1")
    else:
        monkeypatch.delenv("BWAMS_CHAIN_COUNT", raising=False)
    capi.debug_reload()                                       # the switches are read once: say that they changed
    _, gopt = cc.mem_opts(**case.opts)
    b = capi.Batch(ix, len(case.reads), int(case.cum[-1]))
    try:
        b.seed_upload(case.enc, case.cum)
        first = None
        for run in range(3):
            nc, ns = b.chain_run_ert(case.mems, case.mem_off, case.hits, case.hit_off, gopt)
            ch, sd, off = b.chain_fetch()
            assert np.array_equal(off, woff) and nc == len(wch) and ns == len(wsd), run
            for f in CHAIN_FIELDS:
                assert np.array_equal(ch[f], wch[f]), (run, f)
            for f in SEED_FIELDS:
                assert np.array_equal(sd[f], wsd[f]), (run, f)
            got = (ch.tobytes(), sd.tobytes(), off.tobytes())
            if first is None:
                first = got
            assert got == first, run
            cnt = b.debug_chain_counts()
            want = pc.planted_class_counts(planted)
            assert {k: cnt[k] for k in want} == want, (run, cnt)
            for k in cc.COUNT_KEYS:
                if k in COUNTED_ONLY and not count:
                    assert cnt[k] == -1, (run, k)
                else:
                    assert cnt[k] == model[k], (run, k, cnt)
            assert b.debug_chain_lane_counts() == lane_model, run
            assert b.stats().n_chain_redo == model["redo"] == 2, run
    finally:
        b.close()
