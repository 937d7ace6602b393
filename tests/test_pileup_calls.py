"""Rules 10 to 13 of the pileup (include/bwams.h above bwams_pileup_open) on hand-built records: the committed cost tables recomputed
with decimal arithmetic, and bwams/pileup.py's sums, genotype costs, calls and VCF text against values written out here.
tests/test_gpu_pileup_calls.py runs the same records through the C-ABI, tests/test_pileup_vcf_host.py the same calls through
host/pileup_vcf.cpp."""
import os
import re
from decimal import ROUND_HALF_EVEN, Decimal, getcontext

import numpy as np
import pytest

from bwams import pileup
import test_pileup as T
from test_pileup import prec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = range(pileup.GL_MIN_Q, pileup.GL_MAX_Q + 1)


def costs(q: int):
    """rule 12 at 60 digits: -1000 log10(p) of p = 1 - e, p = (1 - e) / 2 + e / 6 and p = e / 3, e = 10^(-q / 10), unrounded"""
    getcontext().prec = 60
    e = Decimal(10) ** (Decimal(-q) / 10)
    return tuple(-1000 * p.log10() for p in (1 - e, (1 - e) / 2 + e / 6, e / 3))


def literals(name: str):
    """the integer literals of the array `name` in csrc/common.h"""
    text = open(os.path.join(ROOT, "bwa-mem-scale_amd", "csrc", "common.h")).read()
    body = re.search(name + r"\[[^\]]*\]\s*=\s*\{([^}]*)\}", text).group(1)
    return tuple(int(x) for x in body.replace("\n", " ").split(","))


def test_tables():
    hom, het = literals("kPileupGlHom"), literals("kPileupGlHet")
    assert len(hom) == len(het) == len(pileup.T_HOM) == len(pileup.T_HET) == 57 == len(QS)
    text = open(os.path.join(ROOT, "bwa-mem-scale_amd", "csrc", "common.h")).read()
    assert re.search(r"kPileupGlMinQ = 4, kPileupGlMaxQ = 60, kPileupGlMis = 477;", text) and pileup.GL_MIS == 477
    for k, q in enumerate(QS):
        exact = costs(q)
        want = [int(x.quantize(Decimal(1), ROUND_HALF_EVEN)) for x in exact]
        assert hom[k] == pileup.T_HOM[k] == want[0], q
        assert het[k] == pileup.T_HET[k] == want[1], q
        assert want[2] == 100 * q + 477, q                                       # the mismatch cost needs no table
        for x in exact:                                                          # no entry near a rounding boundary
            assert abs(x - x.to_integral_value(ROUND_HALF_EVEN)) < Decimal("0.498"), q
    assert pileup.T_HOM[:3] == (220, 165, 126) and pileup.T_HOM[26:] == (0,) * 31 and pileup.T_HET[24:] == (301,) * 33
    assert pileup.GENOTYPES == ((0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3))
    for q in (0, 3, 61, 93):                                                     # 100 q + 477 for every integer q, the clamped ones too
        assert int(costs(q)[2].quantize(Decimal(1), ROUND_HALF_EVEN)) == 100 * q + 477


VCF_HEAD = ("##fileformat=VCFv4.2\n##source=bwams\n%s"
            '##INFO=<ID=DP,Number=1,Type=Integer,Description="Bases counted">\n'
            '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
            '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Bases counted per allele">\n'
            '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Bases counted">\n'
            '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality">\n'
            '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Genotype costs in phred, the least at 0">\n'
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n")
# the worked example of the header: rule 9's seven records (quality 30, MAPQ 60) over c1 = ACGTACGT
EX_SUMS = [[30 * a, 30 * c, 30 * g, 30 * t, 0, 0, 0, 0, 301 * a, 301 * c, 301 * g, 301 * t]
           for a, c, g, t in ((3, 0, 0, 0), (0, 3, 0, 0), (0, 0, 3, 2), (0, 0, 0, 5), (5, 0, 0, 0), (0, 7, 0, 0), (0, 0, 7, 0), (0, 0, 0, 5))]
EX_PL = [159, 159, 159, 64, 64, 54, 95, 95, 0, 89]
EX_VCF = VCF_HEAD % ("##contig=<ID=c1,length=8>\n", "s1") + "c1\t3\t.\tG\tT\t54\t.\tDP=5\tGT:AD:DP:GQ:PL\t0/1:3,2:5:54:54,0,89\n"


def example() -> pileup.Pileup:
    p = pileup.Pileup(T.EX_L_REF)
    p.set_quality()
    assert p.add(b"".join(T.EX_RECS)) == 7
    p.set_ref(0, T.EX_REF)
    return p


def test_worked_example():
    p = example()
    assert p.fetch_quality(0).tolist() == EX_SUMS and p.fetch_quality(0, 2, 3).tolist() == EX_SUMS[2:3]
    assert np.array_equal(p.fetch(0), T.example().fetch(0)) and p.text(T.EX_NAMES) == T.EX_TEXT          # the counters do not know
    calls = p.calls()
    assert len(calls) == 1 and calls[0]["pl"].tolist() == EX_PL
    x = calls[0]
    assert [int(x[f]) for f in ("region", "pos", "ref", "a1", "a2", "qual", "gq", "depth")] == [0, 2, 2, 2, 3, 54, 54, 5]
    assert x["n"].tolist() == [0, 0, 3, 2]
    assert p.vcf(T.EX_NAMES, "s1") == EX_VCF
    assert len(p.calls(min_qual=54)) == 1 and len(p.calls(min_qual=55)) == 0 and len(p.calls(min_depth=6)) == 0
    # cost(GG) = 2 * 3477, cost(GT) = 5 * 301, cost(TT) = 3 * 3477, as the header works them out
    assert [(c - 1505 + 50) // 100 for c in (6954, 1505, 10431)] == [54, 0, 89]


# One reference of 12 bases, T T A N C G A C G T A C; min_baseq 0, min_qual 0, min_depth 2, no_qual_q 25.
HAND_L_REF, HAND_NAMES, HAND_REF = [12], [b"h"], [3, 3, 0, 4, 1, 2, 0, 1, 2, 3, 0, 1]
HAND_OPT = dict(min_qual=0, min_depth=2, no_qual_q=25)
HAND_RECS = [
    prec(0, 0, "1M", "A"), prec(0, 0, "1M", "C"), prec(0, 0, "1M", "G", flag=0x10),      # 0: a tie of A/C, A/G and C/G over T: the lowest g
    prec(0, 1, "1M", "A") * 3 + prec(0, 1, "1M", "C", flag=0x10) * 3,                     # 1: two ALTs over T
    prec(0, 2, "2M", "GG", mapq=17, qual=40) * 4,                                         # 2: MAPQ below the quality: qe 17; hom-alt over A.  3: ref N
    prec(0, 4, "1M", "T"),                                                                # 4: one base: below min_depth
    prec(0, 5, "4M", "AAAA", qual=[0, 3, 61, 93]),                                        # 5..8: clamped to 4 4 60 60
    prec(0, 9, "2M", "CC", qual=None) * 2,                                                # 9 10: no qualities: no_qual_q
]
HAND_SUMS = [[30, 30, 30, 0, 0, 0, 0, 0, 301, 301, 301, 0], [90, 90, 0, 0, 0, 0, 0, 0, 903, 903, 0, 0],
             [0, 0, 68, 0, 0, 0, 36, 0, 0, 0, 1228, 0], [0, 0, 68, 0, 0, 0, 36, 0, 0, 0, 1228, 0], [0, 0, 0, 30, 0, 0, 0, 0, 0, 0, 0, 301],
             [4, 0, 0, 0, 220, 0, 0, 0, 435, 0, 0, 0], [4, 0, 0, 0, 220, 0, 0, 0, 435, 0, 0, 0], [60, 0, 0, 0, 0, 0, 0, 0, 301, 0, 0, 0],
             [60, 0, 0, 0, 0, 0, 0, 0, 301, 0, 0, 0], [0, 50, 0, 0, 0, 2, 0, 0, 0, 604, 0, 0], [0, 50, 0, 0, 0, 2, 0, 0, 0, 604, 0, 0], [0] * 12]
# (pos, ref, a1, a2, qual, gq, depth, n, pl)
HAND_CALLS = [(0, 3, 0, 1, 64, 0, 3, [1, 1, 1, 0], [29, 0, 29, 0, 0, 29, 32, 32, 32, 64]),
              (1, 3, 0, 1, 191, 86, 6, [3, 3, 0, 0], [86, 0, 86, 95, 95, 191, 95, 95, 191, 191]),
              (2, 0, 2, 2, 87, 12, 4, [0, 0, 4, 0], [87, 87, 87, 12, 12, 0, 87, 87, 12, 87]),
              (9, 3, 1, 1, 60, 6, 2, [0, 2, 0, 0], [60, 6, 0, 60, 6, 60, 60, 6, 60, 60]),
              (10, 0, 1, 1, 60, 6, 2, [0, 2, 0, 0], [60, 6, 0, 60, 6, 60, 60, 6, 60, 60])]
HAND_VCF = (VCF_HEAD % ("##contig=<ID=h,length=12>\n", "smp") +
            "h\t1\t.\tT\tA,C\t64\t.\tDP=3\tGT:AD:DP:GQ:PL\t1/2:0,1,1:3:0:64,32,29,32,0,29\n"
            "h\t2\t.\tT\tA,C\t191\t.\tDP=6\tGT:AD:DP:GQ:PL\t1/2:0,3,3:6:86:191,95,86,95,0,86\n"
            "h\t3\t.\tA\tG\t87\t.\tDP=4\tGT:AD:DP:GQ:PL\t1/1:0,4:4:12:87,12,0\n"
            "h\t10\t.\tT\tC\t60\t.\tDP=2\tGT:AD:DP:GQ:PL\t1/1:0,2:2:6:60,6,0\n"
            "h\t11\t.\tA\tC\t60\t.\tDP=2\tGT:AD:DP:GQ:PL\t1/1:0,2:2:6:60,6,0\n")


def hand() -> pileup.Pileup:
    p = pileup.Pileup(HAND_L_REF, min_baseq=0)
    p.set_quality(**HAND_OPT)
    assert p.add(b"".join(HAND_RECS)) == 17
    p.set_ref(0, HAND_REF)
    return p


def as_tuples(calls):
    return [(int(x["pos"]), int(x["ref"]), int(x["a1"]), int(x["a2"]), int(x["qual"]), int(x["gq"]), int(x["depth"]), x["n"].tolist(),
             x["pl"].tolist()) for x in calls]


def test_hand_cases():
    p = hand()
    assert p.fetch_quality(0).tolist() == HAND_SUMS
    # rule 10: min(40, MAPQ 17) = 17, T_HOM[17] = 9 and T_HET[17] = 307, four times; the clamps; a record without qualities
    assert HAND_SUMS[2][2] == 4 * 17 and HAND_SUMS[2][6] == 4 * 9 and HAND_SUMS[2][10] == 4 * 307
    assert as_tuples(p.calls()) == HAND_CALLS and (p.calls()["region"] == 0).all()
    assert p.vcf(HAND_NAMES, "smp") == HAND_VCF
    # the tie at 0: A/C, A/G and C/G cost 2 * 301 + 3477 each; g = 1 wins, and the genotype quality is 0
    assert HAND_CALLS[0][8][1] == HAND_CALLS[0][8][3] == HAND_CALLS[0][8][4] == 0
    assert [int(x) for x in p.calls(min_depth=1)["pos"]] == [0, 1, 2, 4, 5, 7, 8, 9, 10]     # 3 is N; 6 is A over A: no call at any depth
    assert [int(x) for x in p.calls(min_qual=65)["pos"]] == [1, 2]
    p.reset()                                                                    # both planes
    assert not p.c.any() and not p.q.any() and len(p.calls()) == 0
    for part in (HAND_RECS[3:], HAND_RECS[:3]):                                  # any order, any number of calls
        p.add(b"".join(part))
    assert p.fetch_quality(0).tolist() == HAND_SUMS
    with pytest.raises(AssertionError):                                          # set_quality is for zero counters
        p.set_quality()
    q = pileup.Pileup(HAND_L_REF, min_baseq=13)                                  # min_baseq tests the raw byte, before the clamp
    q.set_quality()
    q.add(b"".join(HAND_RECS))
    assert q.fetch_quality(0, 5, 9).tolist() == [[0] * 12] * 2 + HAND_SUMS[7:9]


def test_wrap():
    """the sums are what the device's uint32 hold: a plane set past 2^32 by hand gives the calls of its low 32 bits"""
    p, w = hand(), hand()
    w.q[1] += 1 << 32
    w.c[1, 0] += 1 << 32
    assert w.fetch_quality(0).tolist() == HAND_SUMS and as_tuples(w.calls()) == HAND_CALLS == as_tuples(p.calls())
    w.q[1, pileup.HET + 1] += 1 << 40                                            # a multiple of 2^32 more reads the same
    assert int(w.fetch_quality(0, 1, 2)[0, pileup.HET + 1]) == 903
    # Q[A] near the top at slot 1 (three A, three C): a mismatch of A costs 100 Q[A] + 3 * 477 in 64 bits, which C/C pays; A/C stays
    # the least at 2 * 903, and C/C's pl saturates at 2^31 - 1
    w.q[1, pileup.Q] = (1 << 32) - 10
    x = w.genotypes()[1]
    assert (int(x["a1"]), int(x["a2"])) == (0, 1) and (100 * ((1 << 32) - 10) + 1431 - 1806 + 50) // 100 > 2 ** 31 - 1
    assert x["pl"].tolist() == [86, 0, 2 ** 31 - 1, 95, 2 ** 31 - 1, 2 ** 31 - 1, 95, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1]
    assert int(x["qual"]) == 2 ** 31 - 1 and int(x["gq"]) == 86
    w.q[1, pileup.Q] = 42949672 + (1 << 32)                                      # 100 Q[A] just under 2^32: no saturation, and no wrap of the product
    x = w.genotypes()[1]
    assert int(x["pl"][2]) == (4294967200 + 1431 - 1806 + 50) // 100 == 42949668
    w.c[1, 0] = w.c[1, 5] = (1 << 32) - 1                                        # counters at the top: n and the depth are kept modulo 2^32 ...
    x = w.genotypes()[1]
    assert x["n"].tolist() == [(1 << 32) - 1, (1 << 32) - 1, 0, 0] and int(x["depth"]) == (1 << 32) - 2
    assert 1 in w.calls(min_depth=2 ** 31 - 1)["pos"]                            # ... and compared with min_depth before that
