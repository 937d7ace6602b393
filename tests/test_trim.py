"""bwams/trim.py, the restatement of bwams_fastq_trim's rules T1 to T9 (include/bwams.h), against cases computed by hand from the
rules.  No GPU: the device is compared with this restatement in test_gpu_trim.py."""
import numpy as np
import pytest

from bwams import trim

import trim_cases as tc

CASES = tc.hand_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_case(case):
    _, reads, opt, paired, want = case
    kept, rep, st = trim.trim(reads, opt, paired)
    got = [(int(r["start"]), int(r["len"]), int(r["insert"]), int(r["reason"])) for r in rep]
    assert got == want
    # T7 / T8: the report accounts for every base, the kept reads are the kept intervals, the stats follow from the report
    for r, read in zip(rep, reads):
        assert int(r["removed"].sum()) == len(read[2]) - r["len"]
        assert r["steps"] & 0x3F == sum(1 << k for k in range(6) if r["removed"][k])
    want_kept = [(rd[0], rd[1], rd[2][w[0]:w[0] + w[1]]) for rd, w in zip(reads, want) if w[3] == trim.KEPT]
    assert len(kept) == len(want_kept)
    for k, w in zip(kept, want_kept):
        assert k[0] == w[0] and k[1] == w[1] and np.array_equal(k[2], w[2]) and (k[3] is None or len(k[3]) == len(w[2]))
    assert st["reads_in"] == len(reads) and st["reads_out"] == len(kept) and st["bases_out"] == sum(len(k[2]) for k in kept)
    assert sum(st["dropped"]) == len(reads) - len(kept)
    assert st["pairs_insert"] == (sum(1 for w in want[0::2] if w[2]) if paired else 0)


def test_step_bits_name_the_step_that_cut():
    by = {c[0]: c for c in CASES}
    for name, step in (("t1", trim.S_FIXED), ("t2_front_walk", trim.S_CUT_FRONT), ("t2_walk_one", trim.S_CUT_TAIL),
                       ("t3_below_both", trim.S_OVERLAP), ("t4_remnant_4_cut", trim.S_ADAPTER), ("t5", trim.S_MAX_LEN)):
        _, reads, opt, paired, _ = by[name]
        _, rep, st = trim.trim(reads, opt, paired)
        assert rep["steps"][0] == 1 << step, name
        assert st["step_reads"][step] >= 1 and st["step_bases"][step] == int(rep["removed"][:, step].sum())
        assert sum(st["step_reads"]) == st["step_reads"][step]


def test_longer_than_the_overlap_limit_skips_t3_and_is_counted():
    rng = np.random.default_rng(5)
    reads = tc.named(tc.pair_of(rng, 1025, 1025, 1025) + tc.pair_of(rng, 1024, 1024, 1024), True)
    _, rep, st = trim.trim(reads, trim.identity_opt(overlap=1), True)
    assert [int(x) for x in rep["insert"]] == [0, 0, 1024, 1024]
    assert [int(x) for x in rep["steps"]] == [trim.STEP_SKIPPED, trim.STEP_SKIPPED, 0, 0]
    assert st["pairs_skipped"] == 1 and st["pairs_insert"] == 1


def test_identity():
    reads = tc.bulk(3, 40)
    kept, rep, st = trim.trim(reads, trim.identity_opt(), True)
    assert len(kept) == len(reads)
    for k, r in zip(kept, reads):
        assert k[0] == r[0] and k[1] == r[1] and np.array_equal(k[2], r[2]) and np.array_equal(k[3], r[3])
    assert not rep["steps"].any() and not rep["reason"].any() and st["bases_in"] == st["bases_out"]
    assert trim.to_fastq(kept) == trim.to_fastq(reads)


@pytest.mark.parametrize("field,value", [("cut_window", 0), ("cut_window", 65), ("overlap_min", 0), ("adapter_min_match", 0),
                                         ("adapter_mismatch_per", 0), ("min_len", 0), ("trim_front", -1), ("n_limit", -1),
                                         ("adapter1", b"ACGN"), ("adapter2", b"acgt"), ("adapter1", b"A" * 129)])
def test_refusals_name_the_field(field, value):
    o = trim.Opt()
    setattr(o, field, value)
    with pytest.raises(ValueError, match=field):
        trim.trim([], o, False)


def test_paired_needs_an_even_number_of_reads():
    with pytest.raises(ValueError, match="paired"):
        trim.trim([tc.rd("ACGT")], trim.Opt(), True)


def test_planted_insert_is_found():
    """200 pairs with an insert I in [30, n1 + n2 - 30] and at most 5 errors inside the overlap: I passes, so the largest passing I
    is at least I"""
    rng = np.random.default_rng(17)
    o = trim.identity_opt(overlap=1)
    exact = 0
    for _ in range(200):
        I = int(rng.integers(30, 271))
        a, b = tc.sim_pair(rng, I, 150, 150, err=0.01, max_planted=5)
        got = trim.find_insert(a[2], b[2], o)
        assert got >= I
        exact += got == I
    assert exact >= 190                                      # a larger I passing by chance is rare


def test_all_at_once_searches_equal_the_loops():
    """trim() searches with every candidate at once; the loops written from the rules are the definition"""
    rng = np.random.default_rng(23)
    o = trim.Opt()
    A = trim._codes(tc.ADAPTER)
    for k in range(150):
        n1, n2 = (int(x) for x in rng.integers(1, 200, 2))
        a, b = tc.sim_pair(rng, int(rng.integers(1, 300)), n1, n2, err=0.03, n_frac=0.02)
        assert trim._find_insert_all(a[2], b[2], o) == trim.find_insert(a[2], b[2], o)
        for c in (a[2], b[2]):
            assert trim._find_adapter_all(c, A, o) == trim.find_adapter(c, A, o)
            assert trim._find_adapter_all(c, A[:1 + k % 5], o) == trim.find_adapter(c, A[:1 + k % 5], o)
    for _, reads, opt, paired, _ in CASES:
        if paired:
            for a, b in zip(reads[0::2], reads[1::2]):
                assert trim._find_insert_all(a[2], b[2], opt) == trim.find_insert(a[2], b[2], opt)


def test_to_fastq_text():
    reads = [(b"a", b"x y", tc.codes("ACGTN"), np.frombuffer(b"IIII#", np.uint8)), (b"b", None, tc.codes("AC"), np.frombuffer(b"!~", np.uint8))]
    assert trim.to_fastq(reads) == b"@a x y\nACGTN\n+\nIIII#\n@b\nAC\n+\n!~\n"
    assert trim.to_fastq(reads, with_comment=False) == b"@a\nACGTN\n+\nIIII#\n@b\nAC\n+\n!~\n"
    assert trim.to_fastq([(b"a", b"c", tc.codes("ACGTN"), None)]) == b">a c\nACGTN\n"
