"""The early-exit rule of the banded-SW kernels ("BSW kernel: the early exit") on the CPU: tests/bsw_early_ref.c, the
project's scalar loop with the rule, against the unmodified loop (oracle.loader.bsw_pairs) on more than a million tasks of two
families with fixed seeds.  No task may differ in any of the six outputs, whichever form of the rule runs (after every row, after
every fourth row), the cells computed never exceed the oracle's, and each family is checked not to be degenerate: the rule shortens
at least a tenth of its tasks and leaves at least a tenth untouched."""
import numpy as np
import pytest

from bsw_early import EarlyRef
from oracle import loader
from util import OUT_FIELDS, bsw_sw_opt

ADV_W = tuple(range(1, 21)) + (100, 200)
ADV_PER_GROUP = 15000                  # x 22 band widths x 2 end bonuses = 660 000 tasks
READ_CHUNKS, READ_CAP = 8, 50000       # 8 x ~50 000 = ~400 000 tasks


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return EarlyRef(tmp_path_factory.mktemp("bsw_early"))


def _check(ref, pairs, rq, qq, w, oo, what):
    """-> (tasks, tasks the rule shortened, cells of the oracle, cells with the rule after every row, ... every fourth row)"""
    want, cells = loader.bsw_pairs(pairs, rq, qq, w, oo)
    off, c0, _, r0 = ref.run(pairs, rq, qq, w, oo, 0)
    assert not r0.any() and int(c0.sum()) == cells, what          # the restatement without the rule is the oracle's loop
    out = []
    for mode in (1, 2):
        got, c, rows, _ = ref.run(pairs, rq, qq, w, oo, mode)
        for f in OUT_FIELDS:
            bad = np.flatnonzero(got[f] != want[f])
            assert bad.size == 0, f"{what} mode {mode}: {f} differs at {bad[:5]}: {got[f][bad[:5]]} vs {want[f][bad[:5]]}; {pairs[bad[0]]}"
        assert (c <= c0).all() and int(c.sum()) <= cells, what
        out.append(c)
    for f in OUT_FIELDS:
        assert np.array_equal(off[f], want[f]), (what, f)
    assert (out[0] <= out[1]).all(), what                          # testing less often never computes less
    return len(pairs), int((out[0] < c0).sum()), cells, int(out[0].sum()), int(out[1].sum())


def _not_degenerate(tot, what):
    n, short = tot[0], tot[1]
    print(f"{what}: {n} tasks, the rule shortens {short} ({short / n:.3f}); cells {tot[3] / tot[2]:.3f} of the oracle's after every row, "
          f"{tot[4] / tot[2]:.3f} after every fourth")
    assert short >= n / 10 and n - short >= n / 10, what


def test_read_family(ref):
    oo = bsw_sw_opt(loader)                                        # end_bonus 5, zdrop 100
    tot = np.zeros(5, np.int64)
    for seed in range(READ_CHUNKS):
        pairs, rq, qq = ref.gen_reads(100 + seed, READ_CAP)
        tot += _check(ref, pairs, rq, qq, 100, oo, f"reads seed {seed}")
    assert tot[0] >= 380000
    _not_degenerate(tot, "reads")


def test_adversarial_family(ref):
    tot = np.zeros(5, np.int64)
    for eb in (0, 5):
        oo = bsw_sw_opt(loader, end_bonus=eb)
        for w in ADV_W:
            pairs, rq, qq = ref.gen_adversarial(1000 * eb + w, ADV_PER_GROUP)
            tot += _check(ref, pairs, rq, qq, w, oo, f"adversarial w={w} end_bonus={eb}")
    assert tot[0] == 2 * len(ADV_W) * ADV_PER_GROUP
    _not_degenerate(tot, "adversarial")

