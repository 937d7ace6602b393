"""The toy indexes of tests/sa_dense_cases.py hold what tests/test_gpu_sa_dense.py relies on — shown under the oracle alone, no GPU."""
import numpy as np
import pytest

import sa_dense_cases as cases


@pytest.mark.parametrize("L", cases.SIZES)
def test_row_counts(L):
    _, idx = cases.case(L)
    assert idx.ref_seq_len == 2 * L + 1
    coord, steps, sentinel = cases.walks(L)
    assert len(coord) == 2 * L + 1
    # a row that is a multiple of 8 reads its sample without a step, and is never a sentinel walk
    r8 = np.arange(0, len(coord), 8)
    assert not steps[r8].any() and not sentinel[r8].any()
    # every text position is some row's coordinate: the walks that do not meet the sentinel are a permutation of them but for the quirk
    assert coord.min() >= 0 and coord.max() <= 2 * L + 1


def test_every_case_has_a_sentinel_walk_with_steps():
    """at least one row whose walk meets the sentinel row after one or more LF steps (the flag of the table entry, with a step count)"""
    for L in (31, 100, 2051):
        coord, steps, sentinel = cases.walks(L)
        n = int((sentinel & (steps >= 1)).sum())
        print(f"L = {L}: {int((coord == 0).sum())} rows of value 0, {int(sentinel.sum())} sentinel walks, {n} of them after a step")
        assert n >= 1, f"seed {cases.SEEDS[L]} of L = {L} gives no sentinel walk with a step: pick another seed"


def test_a_walk_longer_than_63_steps():
    """a step count that needs more than six bits, and more steps than a wavefront has lanes"""
    longest = {L: int(cases.walks(L)[1].max()) for L in cases.SIZES}
    print("longest walks:", longest)
    assert max(longest.values()) > 63, f"no walk beyond 63 steps with the seeds {cases.SEEDS}: pick another seed"


def test_planted_motif_gives_strided_rows():
    """max_occ = 3 on the planted genome: an SMEM with s > max_occ, whose rows k + i * (s / max_occ) are no multiples of every stride"""
    sm, coord, off, ctr, opt = cases.oracle_seeds(1000, 3)
    big = sm[sm["s"] > 3]
    assert len(big) >= 1, "no SMEM with more than max_occ occurrences: the motif was not found"
    rows = np.concatenate([r["k"] + np.arange(3) * (r["s"] // 3) for r in big])
    for s in (2, 4):
        assert (rows % s != 0).any(), s
    assert ctr.n_sa_lookups == len(coord) == off[-1]


@pytest.mark.parametrize("L", cases.SIZES)
@pytest.mark.parametrize("stride", (1, 2, 4))
def test_expected_table_layout(L, stride):
    """the packed entries unpack to the walks, entry by entry; the last row is an entry when the stride divides it"""
    t = cases.expected_table(L, stride)
    coord, steps, sentinel = cases.walks(L)
    assert len(t) == (2 * L + 1 + stride - 1) // stride
    r = np.arange(len(t)) * stride
    assert np.array_equal(t >> np.uint64(cases.STEP_SHIFT), steps[r].astype(np.uint64))
    assert np.array_equal((t & cases.SENTINEL) != 0, sentinel[r])
    assert np.array_equal((t & (cases.SENTINEL - np.uint64(1)))[~sentinel[r]], coord[r][~sentinel[r]].astype(np.uint64))
    assert int(steps.max()) < 1 << 23
