"""The batch of tests/chain_plan_cases.py under the oracle alone: it holds a read in every launch of the chaining stage's plan
and on every route behind it, and the seeds counted from its inputs are the seeds planted."""
import numpy as np
import pytest

import chain_cases as cc
import chain_plan_cases as pc


@pytest.fixture(scope="module")
def built():
    case, planted = pc.plan_batch()
    return case, planted, cc.model(case)


def test_seeds_are_the_planted_ones(built):
    case, planted, _ = built
    assert case.notes == list(planted)
    assert cc.seeds_per_read(case).tolist() == [planted[n] for n in case.notes]


def test_a_read_at_both_limits_of_every_wave_class(built):
    case, planted, model = built
    edges = (cc.LANE_SEEDS,) + cc.LDS_CLASSES + (cc.CLASS_XL, cc.CLASS_XL2)
    for lo, hi in zip(edges[:-2], edges[1:-1]):                # S .. L and XL: the class of (lo, hi] has reads of lo + 1 and of hi seeds
        for n in (lo + 1, hi):
            r = case.read("seeds%d" % n)
            assert model["reads"][r][0] == n and cc.tier_of(n)[1] == hi, n
    n, tier = model["reads"][case.read("seeds4097")][0], cc.tier_of(4097)
    assert n == 4097 and tier == ("xl", cc.CLASS_XL2)
    # ... and the class counts the kernel must report follow from the planted counts alone
    want = pc.planted_class_counts(planted)
    assert {k: model[k] for k in want} == want
    assert want["gt_lane"] == len(pc.WAVE_LIMITS) + 2 and want["gt_XL"] == 1 and want["gt_XL2"] == 0      # + equal_in_pass, redo65


def test_the_lane_tier_has_reads_of_every_kind(built):
    case, planted, model = built
    lane = [r for r, n in enumerate(case.notes) if model["reads"][r][3] == "lane"]
    assert len(lane) >= pc.N_LANE + 2
    assert any(len(case.reads[r]) == 0 for r in lane)                                                # no MEM at all
    assert any(len(case.reads[r]) > 0 and planted[case.notes[r]] == 0 for r in lane)                 # a MEM without a hit
    n_lane, gave_up = pc.lc.lane_model(case)
    assert n_lane == len(lane) and gave_up >= 2                                                      # ten_of_10, lane17 (and what the mix holds)
    ten = model["reads"][case.read("ten_of_10")]
    assert ten[:4] == (10, 10, 10, "lane")
    # the lane tier's reads lie between the wave classes' in read order
    first, last = case.read("seeds33"), case.read("seeds4097")
    assert sum(first < r < last for r in lane) >= pc.N_LANE * 3 // 4


def test_the_redo_and_the_heavy_routes(built):
    case, _, model = built
    eq, l17, r65 = (model["reads"][case.read(n)] for n in ("equal_in_pass", "lane17", "redo65"))
    assert eq[3:] == ("lds", True, "heavy") and eq[0] == 41 and eq[2] == 41          # a position twice: chained again (41 chains: the class of 64)
    assert l17[3:] == ("lane", False, "heavy") and l17[2] == 17                      # chain_heavy_kernel's class of 64 chains
    assert r65[3:] == ("lds", True, "heavy") and r65[2] == 65                        # ... and its class of 128
    assert model["redo"] == 2 and model["n_heavy"] >= 3
    assert model["in_wave"] >= len(pc.WAVE_LIMITS) - 1                               # the wave classes' reads filter in their wavefront


def test_the_oracle_chains_every_planted_read(built):
    case, planted, _ = built
    _, _, off = case.oracle()
    kept = np.diff(off)
    for r, n in enumerate(case.notes):
        assert (kept[r] > 0) == (planted[n] > 0), n
