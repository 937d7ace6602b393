"""Rules 14 to 17 of the pileup (include/bwams.h above bwams_pileup_open) on hand-built records: bwams/pileup.py's events, span sums,
alleles, indel calls and VCF texts against values written out here, with the costs worked out beside them, and the properties the
inputs of tests/test_gpu_pileup_indels.py must have before a device result over them means anything.  That file runs the same records
through the C-ABI, tests/test_pileup_indel_vcf_host.py the same calls through host/pileup_indel_vcf.cpp."""
import numpy as np
import pytest

from bwams import pileup
import test_pileup as T
import test_pileup_calls as TC
from test_pileup import prec
from test_depth import OPS

VCF_HEAD = TC.VCF_HEAD.replace('Description="Bases counted">\n##FORMAT=<ID=GT', 'Description="Bases counted">\n'
                               '##INFO=<ID=INDEL,Number=0,Type=Flag,Description="An insertion or deletion, as the CIGARs give it">\n'
                               '##FORMAT=<ID=GT', 1)
assert VCF_HEAD.count("INDEL") == 1

# The worked example of the header: rule 9's seven records (MAPQ 60, so qe = 40: 1, 40, T_HOM = 0, T_HET = 301 a read) over
# c1 = ACGTACGT.  Three 8M reads span slots 0..6, the two 2M1D2M reads at 2 span 2 and 5, the two 2M2I2M reads at 4 span 4 and 6.
EX_SPAN = [[n, 40 * n, 0, 301 * n] for n in (3, 3, 5, 3, 5, 5, 5, 0)]
EX_ALLELES = [(0, 3, 0, 1, 0, 2, 80, 0, 602), (0, 5, 1, 2, 0b1111, 2, 80, 0, 602)]       # a deletion of 1 behind 3; TT inserted behind 5
EX_ROWS = ("c1\t4\t.\tTA\tT\t74\t.\tDP=5;INDEL\tGT:AD:DP:GQ:PL\t0/1:3,2:5:74:74,0,119\n",
           "c1\t6\t.\tC\tCTT\t68\t.\tDP=7;INDEL\tGT:AD:DP:GQ:PL\t0/1:5,2:7:68:68,0,203\n")
EX_HEAD = VCF_HEAD % ("##contig=<ID=c1,length=8>\n", "s1")
EX_INDEL_VCF = EX_HEAD + EX_ROWS[0] + EX_ROWS[1]
EX_VCF_ALL = EX_HEAD + "c1\t3\t.\tG\tT\t54\t.\tDP=5\tGT:AD:DP:GQ:PL\t0/1:3,2:5:54:54,0,89\n" + EX_ROWS[0] + EX_ROWS[1]
CALL_FIELDS = ("region", "pos", "ref", "type", "len", "seq", "gt", "qual", "gq", "depth", "n_ref", "n_alt", "n_other")


def as_tuples(calls):
    return [tuple(int(x[f]) for f in CALL_FIELDS) + (x["pl"].tolist(), bytes(x["del_ref"]).rstrip(b"\0")) for x in calls]


def example() -> pileup.Pileup:
    p = pileup.Pileup(T.EX_L_REF)
    p.set_quality()
    p.set_indels()
    assert p.add(b"".join(T.EX_RECS)) == 7
    p.set_ref(0, T.EX_REF)
    return p


def test_worked_example():
    p = example()
    assert p.fetch_span(0).tolist() == EX_SPAN and p.fetch_span(0, 3, 4).tolist() == EX_SPAN[3:4]
    assert [tuple(int(v) for v in a) for a in p.indel_alleles()] == EX_ALLELES
    # slot 3: cost(RR) = 2 * 4477, cost(RA) = 3 * 301 + 2 * 301, cost(AA) = 3 * 4477; slot 5: 2 * 4477, 7 * 301, 5 * 4477
    assert [(c - 1505 + 50) // 100 for c in (8954, 1505, 13431)] == [74, 0, 119]
    assert [(c - 2107 + 50) // 100 for c in (8954, 2107, 22385)] == [68, 0, 203]
    assert as_tuples(p.indel_calls()) == [(0, 3, 3, 0, 1, 0, 1, 74, 74, 5, 3, 2, 0, [74, 0, 119], b""),        # the deleted base is A: code 0
                                          (0, 5, 1, 1, 2, 15, 1, 68, 68, 7, 5, 2, 0, [68, 0, 203], b"")]
    assert p.indel_vcf(T.EX_NAMES, "s1") == EX_INDEL_VCF and p.vcf_all(T.EX_NAMES, "s1") == EX_VCF_ALL
    assert p.vcf(T.EX_NAMES, "s1") == TC.EX_VCF and p.text(T.EX_NAMES) == T.EX_TEXT                           # what was there does not know
    assert np.array_equal(p.fetch(0), T.example().fetch(0)) and np.array_equal(p.fetch_quality(0), TC.example().fetch_quality(0))
    assert len(p.indel_calls(min_qual=68)) == 2 and len(p.indel_calls(min_qual=69)) == 1 and len(p.indel_calls(min_qual=75)) == 0
    assert [int(x["pos"]) for x in p.indel_calls(min_depth=6)] == [5] and len(p.indel_calls(min_depth=8)) == 0
    p.reset()
    assert not p.fetch_span(0).any() and len(p.indel_alleles()) == 0 and p.indel_vcf(T.EX_NAMES, "s1") == EX_HEAD


# Hand cases over h = ACGTACGTACGTACGT.  Slot 4: three 6M reads at 2 of MAPQ 60 span it (SPAN = 3, 120, 0, 903); two reads delete 5 and
# 6 behind it, one of MAPQ 20 (qe 20: T_HOM 4, T_HET 304) and one of MAPQ 60 (qe 40: 0, 301); one read of MAPQ 3 (qe 4: 220, 435)
# inserts a T there.  ALT is the deletion: n 2, Q 60, HOM 4, HET 605, MIS = 6000 + 954.
#   cost(RR) = 0 + 6954, cost(RA) = 903 + 605 = 1508, cost(AA) = 12000 + 1431 + 4 = 13435: pl 54 0 119, depth 3 + 2 + 1
# Slot 12: no read spans it; two reads of MAPQ 60 insert a C behind it: n 2, Q 80, HOM 0, HET 602.
#   cost(RR) = 8000 + 954 = 8954, cost(RA) = 602, cost(AA) = 0: pl 90 6 0, hom-alt
HAND_L_REF, HAND_NAMES = [16], [b"h"]
HAND_REF = [0, 1, 2, 3] * 4
HAND_RECS = [prec(0, 2, "6M", "GTACGT")] * 3 + [prec(0, 2, "3M2D3M", "GTATAC", mapq=20), prec(0, 2, "3M2D3M", "GTATAC"),
                                                prec(0, 2, "3M1I3M", "GTATCGT", mapq=3), prec(0, 11, "2M1I2M", "TACCG"),
                                                prec(0, 11, "2M1I2M", "TACCG", flag=0x10)]
HAND_ALLELES = [(0, 4, 0, 2, 0, 2, 60, 4, 605), (0, 4, 1, 1, 3, 1, 4, 220, 435), (0, 12, 1, 1, 1, 2, 80, 0, 602)]
HAND_CALLS = [(0, 4, 0, 0, 2, 0, 1, 54, 54, 6, 3, 2, 1, [54, 0, 119], b"\1\2"), (0, 12, 0, 1, 1, 1, 2, 90, 6, 2, 0, 2, 0, [90, 6, 0], b"")]
HAND_VCF = (VCF_HEAD % ("##contig=<ID=h,length=16>\n", "smp") + "h\t5\t.\tACG\tA\t54\t.\tDP=6;INDEL\tGT:AD:DP:GQ:PL\t0/1:3,2:6:54:54,0,119\n"
            "h\t13\t.\tA\tAC\t90\t.\tDP=2;INDEL\tGT:AD:DP:GQ:PL\t1/1:0,2:2:6:90,6,0\n")


def hand() -> pileup.Pileup:
    p = pileup.Pileup(HAND_L_REF)
    p.set_indels()
    assert p.add(b"".join(HAND_RECS)) == len(HAND_RECS)
    p.set_ref(0, HAND_REF)
    return p


def test_hand_cases():
    p = hand()
    assert [(c - 1508 + 50) // 100 for c in (6954, 1508, 13435)] == [54, 0, 119] and [(c + 50) // 100 for c in (8954, 602, 0)] == [90, 6, 0]
    span = p.fetch_span(0).tolist()
    assert span[4] == [3, 120, 0, 903] and span[12] == [0, 0, 0, 0]
    assert span[2] == [6, 3 * 40 + 20 + 40 + 4, 4 + 220, 3 * 301 + 304 + 301 + 435]                       # every read at 2 spans 2 and 3
    assert [tuple(int(v) for v in a) for a in p.indel_alleles()] == HAND_ALLELES
    assert as_tuples(p.indel_calls()) == HAND_CALLS and p.indel_vcf(HAND_NAMES, "smp") == HAND_VCF
    assert [int(x["pos"]) for x in p.indel_calls(min_qual=55)] == [12] and [int(x["pos"]) for x in p.indel_calls(min_depth=3)] == [4]
    # a tie between the deletion and an insertion goes to the deletion (type 0 first); between two sequences to the smaller word
    p = pileup.Pileup(HAND_L_REF)
    p.set_indels()
    p.add(b"".join([prec(0, 2, "3M1I3M", "GTATCGT"), prec(0, 2, "3M1D3M", "GTACGT"), prec(0, 8, "3M1I3M", "ACGGACG"),
                    prec(0, 8, "3M1I3M", "ACGCACG")]))
    p.set_ref(0, HAND_REF)
    calls = as_tuples(p.indel_calls(0, 1))
    assert [c[:6] + c[11:13] for c in calls] == [(0, 4, 0, 0, 1, 0, 1, 1), (0, 10, 2, 1, 1, 1, 1, 1)]
    assert [tie for _, _, tie in p.indel_genotypes()] == [True, True]


def R(rng, refid, pos, cigar, ins=None, **kw):
    """a record with random A C G T; ins: the codes of its first I op's bases"""
    ops, n = [], ""
    for c in cigar:
        if c.isdigit():
            n += c
        else:
            ops.append((int(n), OPS[c]))
            n = ""
    codes, done = [], False
    for n, op in ops:
        if op in (0, 1, 4, 7, 8):
            if op == 1 and ins is not None and not done:
                assert len(ins) == n
                codes += list(ins)
                done = True
            else:
                codes += [int(c) for c in rng.choice([1, 2, 4, 8], n)]
    return prec(refid, pos, ops, codes, **kw)


# The edges of rules 14 and 15, for the device test.  Regions of reference 0: [10, 40) and [40, 60) touch, [100, 150) stands apart;
# reference 1 is its own region to its last position.  Reference base 4 at 130 (an anchor) and at 136 (inside a deletion).
EDGE_L_REF, EDGE_REGIONS, EDGE_NAMES = [200, 50], [(0, 10, 40), (0, 40, 60), (0, 100, 150), (1, 0, 50)], [b"e0", b"e1"]
EDGE_CONFIGS = ({}, {"max_len": 1, "indel_q": 50, "min_qual": 0}, {"indel_q": 0})


def edge_case():
    rng = np.random.default_rng(5)
    r = []
    r += [R(rng, 0, 145, "5M3D5M"), R(rng, 0, 145, "5M3D5M")]                    # anchor 149, the region's last slot; 150..152 lie behind it: OTHER
    r += [R(rng, 0, 145, "5M2I5M"), R(rng, 0, 145, "10M"), R(rng, 0, 140, "10M")]    # an insertion there; [145, 155) spans 149, [140, 150) does not
    r += [R(rng, 0, 70, "5M1I5M"), R(rng, 0, 75, "5M1D5M")]                      # anchors 74 and 79: in no region
    r += [R(rng, 0, 30, "20M"), R(rng, 0, 30, "10M"), R(rng, 0, 35, "5M1I5M"), R(rng, 0, 36, "5M1D9M")]      # over the touching edge at 40; anchors 39 and 40
    r += [R(rng, 1, 40, "15M"), R(rng, 1, 40, "10M"), R(rng, 1, 45, "5M1I3M"), R(rng, 1, 44, "5M1D3M")]      # the last slot: anchor 49; a deletion of 49 behind 48
    r += [R(rng, 0, 12, "2I5M"), R(rng, 0, 12, "2D5M"), R(rng, 0, 12, "2D1I5M")]   # an opening I and D give nothing; the I behind the opening D does
    r += [R(rng, 0, 15, "5M2I3D5M", ins=[1, 2]), R(rng, 0, 15, "5M3D2I5M"), R(rng, 0, 15, "5M2I3D5M", ins=[1, 2])]     # adjacent: two events at 19; one at 19 and one at 22
    r += [R(rng, 0, 20, "5M10N5M"), R(rng, 0, 12, "3M2=1X4M"), R(rng, 0, 25, "2H3S5M1I5M3S"), R(rng, 0, 25, "5M1P5M")]
    for n in (1, 31, 32, 33):
        r += [R(rng, 0, 106, "5M%dI5M" % n)] * 2
    r += [R(rng, 0, 110, "5M2I5M", ins=[1, 15]), R(rng, 0, 110, "5M2I5M", ins=[0, 2])]      # an inserted N, an inserted `=`
    r += [R(rng, 0, 112, "4M3I4M", ins=[1, 2, 8]), R(rng, 0, 111, "5M3I4M", ins=[1, 2, 8])]   # the same allele at 115 from an even and an odd query offset
    for mapq in (0, 3, 41, 60, 255):
        r += [R(rng, 0, 116, "5M1D5M", mapq=mapq), R(rng, 0, 114, "10M", mapq=mapq)]
    r += [R(rng, 0, 116, "5M1D5M", flag=0x400), R(rng, 0, 116, "5M2D5M", flag=0x4)]       # 0x400 and 0x4 are filtered
    r += [R(rng, 0, 126, "5M1D5M")] * 2 + [R(rng, 0, 130, "5M3D5M")] * 2       # reference base 4 at the anchor 130; inside the deletion of 135..137
    r += [R(rng, 0, 100, "1I3M"), R(rng, 0, 99, "1M1D3M"), R(rng, 0, 0, "0M2I4M"),R(rng, 0, 140, "3M0I0D3M")]
    ref = [rng.integers(0, 4, n).astype(np.uint8) for n in EDGE_L_REF]
    ref[0][[130, 136]] = 4
    return r, ref


def edge(**opt) -> pileup.Pileup:
    recs, ref = edge_case()
    p = pileup.Pileup(EDGE_L_REF, EDGE_REGIONS, min_mapq=opt.pop("min_mapq", 0))
    p.set_quality()
    p.set_indels(**opt)
    p.add(b"".join(recs))
    p.set_ref_genome(ref)
    return p


def alleles_at(p, region, pos):
    return [tuple(int(a[f]) for f in ("type", "len", "n")) for a in p.indel_alleles() if (int(a["region"]), int(a["pos"])) == (region, pos)]


def test_edges():
    p = edge()
    D, I, O = pileup.EV_DEL, pileup.EV_INS, pileup.EV_OTHER
    assert alleles_at(p, 2, 149) == [(I, 2, 1), (O, 0, 2)]                       # the deletions reach past the region
    span = p.fetch_span(2)
    assert span[49].tolist() == [1, 40, 0, 301] and span[48, 0] == 5            # only [145, 155) spans 149
    assert not any(int(a["pos"]) in (74, 79) for a in p.indel_alleles())
    assert alleles_at(p, 0, 39) == [(I, 1, 1)] and alleles_at(p, 1, 40) == [(D, 1, 1)]
    # 39: [30, 50) and [36, 41); 40: [30, 50) and [40, 45), the touching regions' edge between them; 38: [30, 40), [35, 40) and the [35, 40) behind the N skip too
    assert p.fetch_span(0)[29].tolist() == [2, 80, 0, 602] and p.fetch_span(1)[0, 0] == 2 and p.fetch_span(0)[28, 0] == 5
    assert alleles_at(p, 3, 49) == [(I, 1, 1)] and alleles_at(p, 3, 48) == [(D, 1, 1)]      # 49, the reference's last position, is deleted
    assert p.fetch_span(3)[49, 0] == 1 and p.fetch_span(3)[48, 0] == 3
    assert alleles_at(p, 0, 13) == [(I, 1, 1)] and alleles_at(p, 0, 11) == [] and alleles_at(p, 0, 12) == []
    assert alleles_at(p, 0, 19) == [(D, 3, 3), (I, 2, 2)] and alleles_at(p, 0, 22) == [(I, 2, 1)]
    assert [g[:2] for g in alleles_at(p, 2, 110)] == [(I, 1), (I, 31), (I, 32), (O, 0)] and alleles_at(p, 2, 110)[3][2] == 2
    assert alleles_at(p, 2, 114) == [(O, 0, 2)]                                  # an inserted N, an inserted `=`
    assert alleles_at(p, 2, 115) == [(I, 3, 2)] and int(p.indel_alleles()[[int(a["pos"]) == 115 for a in p.indel_alleles()]][0]["seq"]) == 0b110100
    assert alleles_at(p, 2, 120) == [(D, 1, 5)]
    a = p.indel_alleles()[[int(a["pos"]) == 120 for a in p.indel_alleles()]][0]
    assert (int(a["q"]), int(a["hom"]), int(a["het"])) == (4 + 4 + 40 * 3, 220 * 2, 435 * 2 + 301 * 3)     # MAPQ 0 3 | 41 60 255
    assert alleles_at(p, 2, 130) == [(D, 1, 2)] and 130 not in [int(c["pos"]) for c in p.indel_calls(0, 1)]
    c = [c for c in p.indel_calls(0, 1) if int(c["pos"]) == 134][0]
    assert c["del_ref"][:3].tolist()[1] == 4 and "N" in p.indel_vcf(EDGE_NAMES, "s", 0, 1)
    assert alleles_at(p, 2, 100) == [] and alleles_at(p, 2, 142) == [(D, 0, 1), (I, 0, 1)]
    q = edge(max_len=1, indel_q=50, min_qual=0, min_mapq=2)
    assert alleles_at(q, 2, 110) == [(I, 1, 2), (O, 0, 6)] and alleles_at(q, 0, 19) == [(O, 0, 5)]
    a = q.indel_alleles()[[int(a["pos"]) == 120 for a in q.indel_alleles()]][0]
    assert (int(a["n"]), int(a["q"])) == (4, 4 + 41 + 50 + 50)                  # MAPQ 0 is filtered; 3 41 60 255 under indel_q 50
    assert (pileup.Pileup(EDGE_L_REF, EDGE_REGIONS).c == 0).all()


def ins_channel_holds(p: pileup.Pileup):
    """the invariant: at every slot the events that come from an I op, whatever their type, are the INS channel"""
    n = np.zeros(p.n_slots, np.int64)
    for s, _, _, _, _, from_ins in p.events:
        n[s] += from_ins
    return np.array_equal(n, p.c[:, pileup.INS])


# The random input of the device test: reads of 60 to 120 bases over regions with gaps, a share of them with one I or D at one of a few
# dozen sites so that alleles repeat; planted at the end: three reads each of two insertions at one anchor (a tie).
RAND_L_REF, RAND_REGIONS, RAND_NAMES = [3000, 1200], [(0, 100, 1100), (0, 1100, 1500), (0, 1700, 2900), (1, 50, 1150)], [b"r0", b"r1"]


def random_case(seed: int, n_rec: int = 2500):
    rng = np.random.default_rng(seed)
    sites = [(int(rng.integers(0, 2)), int(rng.integers(80, 2950)), "ID"[int(rng.integers(0, 2))], int(rng.choice([1, 1, 2, 3, 5, 12, 32, 33, 40])),
              [int(c) for c in rng.choice([1, 2, 4, 8, 15], 40, p=[.245, .245, .245, .245, .02])]) for _ in range(60)]
    recs = []
    for _ in range(n_rec):
        mapq, flag = int(rng.choice([0, 3, 20, 41, 60, 255])), int(rng.choice([0, 0, 0, 16, 16, 0x400, 0x800]))
        if rng.random() < 0.4:
            refid, at, op, n, ins = sites[int(rng.integers(0, len(sites)))]
            if rng.random() < 0.15:
                n = int(rng.integers(1, 4))                                      # another allele at the same anchor
            a, b = int(rng.integers(1, 60)), int(rng.integers(1, 60))
            cigar = "%dM%d%s%dM" % (a, n, op, b) if rng.random() < 0.9 else "3S%dM%d%s%dM2N4M" % (a, n, op, b)
            recs.append(R(rng, refid, at - a + 1, cigar, ins=ins[:n] if op == "I" else None, mapq=mapq, flag=flag))
        else:
            n = int(rng.integers(60, 121))
            recs.append(R(rng, int(rng.integers(0, 2)), int(rng.integers(0, 2990)), "%dM" % n, mapq=mapq, flag=flag))
    recs += [R(rng, 0, 495, "5M2I5M", ins=[1, 2])] * 3 + [R(rng, 0, 495, "5M2I5M", ins=[8, 8])] * 3
    ref = [rng.choice([0, 1, 2, 3, 4], n, p=[.2425, .2425, .2425, .2425, .03]).astype(np.uint8) for n in RAND_L_REF]
    ref[0][499] = 0
    return recs, ref


def random_model(seed: int, adds=1, reverse=False) -> pileup.Pileup:
    recs, ref = random_case(seed)
    recs = recs[::-1] if reverse else recs
    p = pileup.Pileup(RAND_L_REF, RAND_REGIONS)
    p.set_quality()
    p.set_indels()
    for k in range(adds):
        p.add(b"".join(recs[k * len(recs) // adds:(k + 1) * len(recs) // adds]))
    p.set_ref_genome(ref)
    return p


@pytest.mark.parametrize("seed", (1, 2))
def test_random_inputs_say_something(seed):
    """before any device claim over these inputs: they give calls of both types, OTHER events and a tie (hom-alt calls: the hand cases)"""
    p = random_model(seed)
    calls, alleles = p.indel_calls(), p.indel_alleles()
    assert {int(c["type"]) for c in calls} == {0, 1} and len(calls) >= 20
    assert (alleles["type"] == pileup.EV_OTHER).sum() >= 1 and (calls["n_other"] > 0).any()
    assert any(tie for _, _, tie in p.indel_genotypes()) and len(p.calls()) >= 1
    assert any(c["del_ref"].max() == 4 for c in calls) or seed != 1
    assert ins_channel_holds(p)
    # accumulation: the order and the number of adds do not matter
    q, r = random_model(seed, adds=5), random_model(seed, reverse=True)
    for other in (q, r):
        assert np.array_equal(other.span, p.span) and other.indel_alleles().tobytes() == alleles.tobytes()
        assert other.vcf_all(RAND_NAMES, "s") == p.vcf_all(RAND_NAMES, "s")


def test_invariant_and_refusal():
    for p in (example(), hand(), edge()):
        assert ins_channel_holds(p)
    p = hand()
    before = (p.span.copy(), list(p.events), p.c.copy())
    with pytest.raises(pileup.PileupRefusal):
        p.add(prec(0, 2, "3M1I3M", "GTATCGT") + prec(0, 2, "3M1I3M", "GTATCG"))    # rule 3: the second record's CIGAR asks for 7 bases
    assert np.array_equal(p.span, before[0]) and p.events == before[1] and np.array_equal(p.c, before[2])
