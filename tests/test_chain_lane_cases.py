"""The planted reads of tests/chain_lane_cases.py under the oracle alone: every case sits where it was aimed (seed counts, nine
and ten chains before the filter, repeated positions, merged / separate / skipped seeds, kept chains), so that
tests/test_gpu_chain_lane.py compares the lane tier with the oracle on the inputs it believes it does."""
import numpy as np
import pytest

import chain_cases as cc
import chain_lane_cases as lc


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_case_has_its_property(name):
    case = lc.CASES[name]()
    ch, sd, off = case.oracle(do_flt=False)
    kch, _, koff = case.oracle()
    ns = cc.seeds_per_read(case)
    for note, what in case.expect.items():
        r = case.read(note)
        lo, hi = int(off[r]), int(off[r + 1])
        if what[0] == "chains":
            assert hi - lo == what[1], (name, note, hi - lo)
        elif what[0] == "seeds":
            assert int(ch["n"][lo:hi].sum()) == what[1] < ns[r], (name, note)
        elif what[0] == "repeat":
            assert len(np.unique(ch["pos"][lo:hi])) < hi - lo <= lc.LEAF_CHAINS, (name, note)
        elif what[0] == "kept":
            assert int(koff[r + 1] - koff[r]) == what[1] and hi - lo == 3, (name, note)
        else:
            raise AssertionError(what)


def test_seed_counts_are_the_ones_aimed_at():
    c = lc.seed_counts()
    assert cc.seeds_per_read(c).tolist() == list(lc.SEED_COUNTS) + [0]
    assert lc.lane_model(c) == (len(lc.SEED_COUNTS), 0)


def test_leaf_full_gives_up_at_the_tenth_chain_only():
    c = lc.leaf_full()
    assert cc.seeds_per_read(c).tolist() == [10, 10, 32, 32]
    assert [lc.lane_model(lc.one(c, n))[1] for n in c.notes] == [0, 1, 0, 1]
    # ten_of_32: the tenth chain is started by the read's last seed, after 27 seeds were linked into the nine others
    ch, sd, off = lc.one(c, "ten_of_32").oracle(do_flt=False)
    assert sorted(ch["n"].tolist()) == [1] + [3] * 5 + [4] * 4


def test_equal_keys_fill_the_leaf():
    c = lc.equal_keys()
    _, _, off = c.oracle(do_flt=False)
    nk = dict(zip(c.notes, np.diff(off).tolist()))
    assert nk["two_same"] == 6 and nk["three_same"] == 7 and nk["three_same_full"] == 9
    assert all(nk["%s_%s" % (s, h)] == 9 for s in ("first", "mid", "last") for h in ("asc", "desc", "rand"))


def test_weight_floor_drops_all_some_none():
    kept = {}
    for w in ("all", "some", "none"):
        c = lc.weight_floor(w)
        _, _, off = c.oracle(do_flt=False)
        assert np.diff(off).tolist() == [9, 2]
        ch, _, koff = c.oracle()
        kept[w] = np.diff(koff).tolist()
    assert kept["all"] == [1, 1]                                  # a_[0] stays
    assert kept["none"][0] > kept["some"][0] > 1 and kept["some"][1] == 1 and kept["none"][1] == 2


def test_tie_sort_has_ties_and_dropped_chains():
    c = lc.tie_sort()
    ch, sd, off = c.oracle(do_flt=False)
    w = cc.chain_weights(ch, sd)
    r = c.read("nine_equal")
    assert len(set(w[off[r]:off[r + 1]].tolist())) == 1 and off[r + 1] - off[r] == 9
    r = c.read("tied_under_dominant")
    _, _, koff = c.oracle()
    assert off[r + 1] - off[r] == 9 and koff[r + 1] - koff[r] < 9
    for n in range(3, 10):
        r = c.read("adversary%d" % n)
        assert off[r + 1] - off[r] == n


@pytest.mark.parametrize("n,wave", [(63, 0), (64, 0), (65, 0), (200, 0), (200, 7)])
def test_batches_hold_every_seed_count_and_a_few_give_ups(n, wave):
    c = lc.batch(n, wave)
    ns = cc.seeds_per_read(c)
    assert len(ns) == n and ns[0] == 0 and ns[-1] == 0 and (ns[1:-1] == 0).sum() >= 3
    lane, gave_up = lc.lane_model(c)
    assert (lane < n) == bool(wave) and 0 < gave_up < lane // 4
    if n == 200:
        assert set(range(1, 33)) <= set(ns.tolist())
    if wave:
        assert (ns > cc.LANE_SEEDS).sum() >= n // wave - 1
