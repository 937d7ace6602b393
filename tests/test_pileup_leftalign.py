"""Rule 18 of the pileup (include/bwams.h above bwams_pileup_open): the left-alignment of the indel store's events in bwams/pileup.py,
pinned from first principles, because nothing else restates it.  A brute force over random references rich in repeats applies every
stored event to its reference and asks that the haplotype is the one the CIGAR gave and that no anchor further left in the region
gives it too; hand cases have their alleles, span sums and VCF rows written out.  The builders of tests/test_gpu_pileup_leftalign.py's
inputs live here as well, with the properties those inputs must have before a device result over them means anything."""
import numpy as np
import pytest

from bwams import pileup
import test_pileup as T
import test_pileup_indels as TI
from test_pileup import prec
from test_depth import OPS

D, I, O = pileup.EV_DEL, pileup.EV_INS, pileup.EV_OTHER
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}


def codes(text: str) -> np.ndarray:
    return np.array([CODE[c] for c in text], np.uint8)


def seq_word(text: str) -> int:
    return sum(CODE[c] << (2 * j) for j, c in enumerate(text))


def ops_of(cigar: str):
    out, n = [], ""
    for c in cigar:
        if c.isdigit():
            n += c
        else:
            out.append((int(n), OPS[c]))
            n = ""
    return out


def rd(ref, refid, pos, cigar, ins="", **kw):
    """a record whose match bases are the reference's (A for an N) and whose I ops take their letters from `ins` in turn"""
    letters, x, at = [], pos, 0
    for n, op in ops_of(cigar):
        if op in (0, 7, 8):
            letters += ["ACGTA"[int(c)] for c in ref[refid][x:x + n]]
        elif op == 1:
            letters += list(ins[at:at + n])
            at += n
        elif op == 4:
            letters += ["G"] * n
        if op in (0, 2, 3, 7, 8):
            x += n
    assert at == len(ins)
    return prec(refid, pos, cigar, "".join(letters), **kw)


def model(l_ref, regions, ref, adds, leftalign=True, quality=False, opt=None, **kw) -> pileup.Pileup:
    """the restatement after the adds, the reference in place before them as rule 18 wants it; leftalign None: the call is never made"""
    p = pileup.Pileup(l_ref, regions, **kw)
    if quality:
        p.set_quality()
    p.set_indels(**(opt or {}))
    if leftalign is not None:
        p.set_indel_leftalign(leftalign)
    p.set_ref_genome(ref)
    for d in adds:
        p.add(d)
    return p


def shifts(l_ref, regions, ref, adds, **kw):
    """[(the CIGAR's event, the stored event, the shift)] for every event, in the order of the records"""
    on, off = model(l_ref, regions, ref, adds, True, **kw), model(l_ref, regions, ref, adds, False, **kw)
    assert len(on.events) == len(off.events)
    return [(a, b, a[0] - b[0]) for a, b in zip(off.events, on.events)]


def alleles(p):
    return [tuple(int(v) for v in a) for a in p.indel_alleles()]


# ---- the brute force ----------------------------------------------------------------------------------------------------------------
def repeat_rich(rng, n: int) -> np.ndarray:
    """random bases between tracts of a unit of 1 to 5 bases repeated 2 to 12 times, and an N about every 60 bases"""
    out = []
    while len(out) < n:
        if rng.random() < 0.7:
            out += [int(c) for c in rng.integers(0, 4, int(rng.integers(1, 6)))] * int(rng.integers(2, 13))
        else:
            out += [int(c) for c in rng.integers(0, 4, int(rng.integers(1, 8)))]
    ref = np.array(out[:n], np.uint8)
    ref[rng.random(n) < 1 / 60] = 4
    return ref


def tokens(ref):
    """an N matches nothing, itself included: every N of the reference is a letter of its own"""
    return [int(c) if c < 4 else ("N", p) for p, c in enumerate(ref)]


def haplotype(tok, a: int, kind: int, n: int, seq):
    """the reference with the event applied; seq: the inserted letters as a list"""
    return tok[:a + 1] + tok[a + 1 + n:] if kind == D else tok[:a + 1] + list(seq) + tok[a + 1:]


def brute_case(seed: int):
    rng = np.random.default_rng(seed)
    l_ref = [400, 260]
    ref = [repeat_rich(rng, n) for n in l_ref]
    regions = [(0, 20, 150), (0, 150, 230), (0, 260, 400), (1, 0, 260)]           # two touch; reference 1 from its position 0
    recs = []
    for _ in range(260):
        r = int(rng.integers(0, 2))
        a, b, n = int(rng.integers(1, 30)), int(rng.integers(1, 30)), int(rng.choice([1, 1, 2, 2, 3, 4, 5, 6, 10]))
        pos = int(rng.integers(0, l_ref[r] - a - b - n))
        if rng.random() < 0.5:
            recs.append(rd(ref, r, pos, "%dM%dD%dM" % (a, n, b), mapq=int(rng.choice([20, 60]))))
        else:                                                                     # mostly a copy of what follows the anchor: it can move
            follows = ref[r][pos + a:pos + a + n]
            ins = "".join("ACGT"[int(c)] for c in (follows if rng.random() < 0.8 and (follows < 4).all() else rng.integers(0, 4, n)))
            recs.append(rd(ref, r, pos, "%dM%dI%dM" % (a, n, b), ins))
    return l_ref, regions, ref, recs


@pytest.mark.parametrize("seed", (1, 2, 4))
def test_brute_force(seed):
    l_ref, regions, ref, recs = brute_case(seed)
    pairs = shifts(l_ref, regions, ref, [b"".join(recs)])
    probe = pileup.Pileup(l_ref, regions)
    assert len(pairs) > 150
    moved = 0
    for (s0, kind, n, seq0, qe, from_ins), (s1, kind1, n1, seq1, qe1, from_ins1), k in pairs:
        assert (kind, n, qe, from_ins) == (kind1, n1, qe1, from_ins1) and k >= 0
        if kind == O:                                                             # a deletion that leaves its region: stored as rule 14 has it
            assert (s1, seq1) == (s0, seq0)
            continue
        region, a0 = probe._place(s0)
        region1, a1 = probe._place(s1)
        r, beg, _ = regions[region]
        assert region1 == region and a1 == a0 - k and a1 >= beg                   # inside the anchor's region
        tok = tokens(ref[r])
        letters = lambda word: [word >> (2 * j) & 3 for j in range(n)]
        want = haplotype(tok, a0, kind, n, letters(seq0))
        assert haplotype(tok, a1, kind, n, letters(seq1)) == want                # the same haplotype ...
        if kind == D:
            assert seq1 == 0
        for c in range(beg, a1):                                                  # ... and no anchor further left in the region gives it
            assert haplotype(tok, c, kind, n, want[c + 1:c + 1 + n]) != want, (s0, kind, n, c)
        moved += k > 0
    assert moved > 60 and any(k > n for (_, _, n, _, _, _), _, k in pairs) and any(k == 0 for _, _, k in pairs)
    stops = [probe._place(b[0]) for _, b, k in pairs if k > 0]
    assert any(a == regions[reg][1] for reg, a in stops)                          # one stopped at its region's first slot
    assert any(ref[regions[reg][0]][a] == 4 for reg, a in stops)                  # and one at an N


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------
# A^10 behind GC: a one-base deletion at each of the ten positions 2..11 of the tract, every read 16 long from 0, MAPQ 60 (qe 40: 1, 40,
# 0, 301 a read).  All ten become the deletion of position 2 behind the C at 1.  The read that deletes p spanned 0..p-2 and p+1..14; its
# first run ended at the anchor p - 1 and loses the slots 1..p-2, so it spans slot 0 and p+1..14: slot s >= 3 has the reads with p < s.
A10_L_REF, A10_NAMES = [16], [b"t"]
A10_REF = codes("GC" + "A" * 10 + "TGCA")
A10_RECS = [rd([A10_REF], 0, 0, "%dM1D%dM" % (p, 15 - p)) for p in range(2, 12)]
A10_SPAN_N = [10, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10, 10, 0]
A10_ALLELES = [(0, 1, D, 1, 0, 10, 400, 0, 3010)]
# slot 1: no read spans it.  cost(RR) = 10 * 4477, cost(RA) = 3010, cost(AA) = 0
A10_VCF = (TI.VCF_HEAD % ("##contig=<ID=t,length=16>\n", "s") + "t\t2\t.\tCA\tC\t448\t.\tDP=10;INDEL\tGT:AD:DP:GQ:PL\t1/1:0,10:10:30:448,30,0\n")
# Without the rule: ten alleles of n 1 at the anchors 1..10.
A10_OFF_ANCHORS = list(range(1, 11))


def test_homopolymer_a10():
    p = model(A10_L_REF, (), [A10_REF], [b"".join(A10_RECS)])
    assert [(44770 + 50) // 100, (3010 + 50) // 100] == [448, 30]
    assert p.fetch_span(0).tolist() == [[n, 40 * n, 0, 301 * n] for n in A10_SPAN_N]
    assert alleles(p) == A10_ALLELES and p.indel_vcf(A10_NAMES, "s") == A10_VCF
    assert np.array_equal(p.fetch(0)[:, pileup.DEL], [0, 0] + [1] * 10 + [0] * 4)                 # rule 4's channel stays with the CIGARs
    off = model(A10_L_REF, (), [A10_REF], [b"".join(A10_RECS)], False)
    never = model(A10_L_REF, (), [A10_REF], [b"".join(A10_RECS)], None)
    for q in (off, never):
        assert [(a[1], a[5]) for a in alleles(q)] == [(x, 1) for x in A10_OFF_ANCHORS]
        assert np.array_equal(q.fetch(0), p.fetch(0))
    assert off.indel_vcf(A10_NAMES, "s") == never.indel_vcf(A10_NAMES, "s") != A10_VCF


# (CA)^8 between GT and GT: C at the even positions 2..16, A at the odd ones.  Three deletions of two bases: CA behind the A at 9, AC
# behind the C at 4, CA behind the A at 13: shifts of 8, 3 and 12, all to the T at 1.  Two insertions: CA behind the A at 7 (a shift of
# 6, three times its length, the sequence as it was) and AC behind the C at 6 (a shift of 5: the sequence rotated by one to CA).
CA8_L_REF, CA8_NAMES = [20], [b"u"]
CA8_REF = codes("GT" + "CA" * 8 + "GT")
CA8_RECS = [rd([CA8_REF], 0, 0, "10M2D8M"), rd([CA8_REF], 0, 0, "5M2D13M"), rd([CA8_REF], 0, 0, "14M2D4M"),
            rd([CA8_REF], 0, 0, "8M2I12M", "CA"), rd([CA8_REF], 0, 0, "7M2I13M", "AC")]
CA8_SHIFTS = [8, 3, 12, 6, 5]
CA8_ALLELES = [(0, 1, D, 2, 0, 3, 120, 0, 903), (0, 1, I, 2, seq_word("CA"), 2, 80, 0, 602)]
# Every first run began at 0 and ended at the old anchor: each read spans slot 0 and nothing up to its old anchor; behind the event
# 12..18, 7..18 and 16..18 for the deletions, 8..18 and 7..18 for the insertions.
CA8_SPAN_N = [5, 0, 0, 0, 0, 0, 0, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 0]
# slot 1: ALT is the deletion (n 3), the two insertions are n_other.  cost(RR) = 3 * 4477, cost(RA) = 903, cost(AA) = 0
CA8_VCF = (TI.VCF_HEAD % ("##contig=<ID=u,length=20>\n", "s") + "u\t2\t.\tTCA\tT\t134\t.\tDP=5;INDEL\tGT:AD:DP:GQ:PL\t1/1:0,3:5:9:134,9,0\n")


def test_dinucleotide_ca8():
    data = [b"".join(CA8_RECS)]
    assert [k for _, _, k in shifts(CA8_L_REF, (), [CA8_REF], data)] == CA8_SHIFTS
    p = model(CA8_L_REF, (), [CA8_REF], data)
    assert [(13431 + 50) // 100, (903 + 50) // 100] == [134, 9]
    assert alleles(p) == CA8_ALLELES and p.fetch_span(0)[:, 0].tolist() == CA8_SPAN_N
    assert p.indel_vcf(CA8_NAMES, "s") == CA8_VCF
    assert p.indel_calls()[0]["del_ref"][:3].tolist() == [1, 0, 0]                 # del_ref from the shifted anchor: C A
    assert np.array_equal(p.fetch(0)[:, pileup.INS], [0] * 6 + [1, 1] + [0] * 12)  # the INS channel stays at 6 and 7


# The header's examples.  Rule 9's seven records over c1 = ACGTACGT repeat nothing, so rule 17's two rows stand.  c2 = TCAAAAGT with an
# 8M read and two one-base deletions behind 4 and behind 2: one allele behind the C at 1, which only the 8M read spans.
#   cost(RR) = 2 * 4477 = 8954, cost(RA) = 301 + 602 = 903, cost(AA) = 4477: pl 81 0 36
C2_L_REF, C2_NAMES, C2_REF = [8], [b"c2"], codes("TCAAAAGT")
C2_RECS = [rd([C2_REF], 0, 0, "8M"), rd([C2_REF], 0, 0, "5M1D2M"), rd([C2_REF], 0, 0, "3M1D4M")]
C2_SPAN_N = [3, 1, 1, 1, 2, 2, 3, 0]
C2_ROW = "c2\t2\t.\tCA\tC\t81\t.\tDP=3;INDEL\tGT:AD:DP:GQ:PL\t0/1:1,2:3:36:81,0,36\n"
C2_OFF_ROWS = ("c2\t3\t.\tAA\tA\t36\t.\tDP=3;INDEL\tGT:AD:DP:GQ:PL\t0/1:2,1:3:36:36,0,81\n",
               "c2\t5\t.\tAA\tA\t36\t.\tDP=3;INDEL\tGT:AD:DP:GQ:PL\t0/1:2,1:3:36:36,0,81\n")
C2_HEAD = TI.VCF_HEAD % ("##contig=<ID=c2,length=8>\n", "s1")


def test_worked_examples():
    ex = model(T.EX_L_REF, (), [np.array(T.EX_REF, np.uint8)], [b"".join(T.EX_RECS)], quality=True)
    assert ex.fetch_span(0).tolist() == TI.EX_SPAN and alleles(ex) == TI.EX_ALLELES
    assert ex.indel_vcf(T.EX_NAMES, "s1") == TI.EX_INDEL_VCF and ex.vcf_all(T.EX_NAMES, "s1") == TI.EX_VCF_ALL
    assert [(c - 903 + 50) // 100 for c in (8954, 903, 4477)] == [81, 0, 36]
    p = model(C2_L_REF, (), [C2_REF], [b"".join(C2_RECS)])
    assert p.fetch_span(0)[:, 0].tolist() == C2_SPAN_N and alleles(p) == [(0, 1, D, 1, 0, 2, 80, 0, 602)]
    assert p.indel_vcf(C2_NAMES, "s1") == C2_HEAD + C2_ROW
    off = model(C2_L_REF, (), [C2_REF], [b"".join(C2_RECS)], False)
    assert off.indel_vcf(C2_NAMES, "s1") == C2_HEAD + C2_OFF_ROWS[0] + C2_OFF_ROWS[1]


def test_refusals_and_the_option_s_life():
    p = pileup.Pileup(C2_L_REF)
    with pytest.raises(AssertionError):
        p.set_indel_leftalign()                                                   # no store
    p.set_indels()
    with pytest.raises(AssertionError):
        p.set_indel_leftalign(2)
    p.set_indel_leftalign()
    with pytest.raises(AssertionError):
        p.add(C2_RECS[0])                                                         # the region's reference is not set
    assert not p.c.any() and not p.dirty
    p.set_ref(0, C2_REF)
    p.add(b"".join(C2_RECS))
    with pytest.raises(AssertionError):
        p.set_ref(0, C2_REF)                                                      # after an add
    with pytest.raises(AssertionError):
        p.set_indel_leftalign(False)
    p.reset()
    assert p.leftalign and p.ref_set == [True]
    p.set_ref(0, C2_REF)                                                          # legal again
    p.add(b"".join(C2_RECS))
    assert alleles(p) == [(0, 1, D, 1, 0, 2, 80, 0, 602)]
    p.reset()
    p.set_indels()                                                                # replaces the store's options: off
    assert not p.leftalign
    q = pileup.Pileup(C2_L_REF)                                                   # neither refusal on another handle
    q.set_indels()
    q.add(b"".join(C2_RECS))
    q.set_ref(0, C2_REF)
    assert [a[1] for a in alleles(q)] == [2, 4]


# ---- the device test's inputs -----------------------------------------------------------------------------------------------------------
def _tract(unit: str, n: int) -> str:
    return (unit * (n // len(unit) + 1))[:n]


# Shifts that cross the align kernel's 64-position step.  A tract of S + 1 A between C and G: the deletion of its last A moves by S,
# the insertion of an A behind its last A by S + 1.  Then a 200-base homopolymer and a 300-base (CA)n.
STEP_SHIFTS = (63, 64, 65, 128, 129)


def step_case():
    text, at = "TG", {}
    for s in STEP_SHIFTS:
        at[s] = len(text) + 1                                                     # the tract's first position, behind a C
        text += "C" + "A" * (s + 1) + "GT"
    at["T200"] = len(text) + 1
    text += "G" + "T" * 200 + "CG"
    at["CA300"] = len(text) + 1
    text += "T" + _tract("CA", 300) + "TTG"
    ref = [codes(text)]
    recs = []
    for s in STEP_SHIFTS:
        t = at[s]
        recs += [rd(ref, 0, t - 2, "%dM1D2M" % (s + 2)), rd(ref, 0, t + s - 4, "5M1I2M", "A"), rd(ref, 0, t + s - 3, "3M1D2M", mapq=20)]
    t = at["T200"]
    for k, n in ((198, 1), (150, 2), (100, 3), (70, 1), (64, 2), (10, 5)):           # n bases behind the tract's base k, all inside it
        recs += [rd(ref, 0, t + k - 4, "5M%dD3M" % n), rd(ref, 0, t - 1, "%dM%dI3M" % (k + 2, n), "T" * n)]
    t = at["CA300"]
    for k, n, ins in ((297, 2, "CA"), (280, 4, "ACAC"), (131, 2, "AC"), (130, 2, "CA"), (66, 6, "CACACA"), (65, 2, "AC"), (3, 2, "AC")):
        ins = ins if ins[0] == "CA"[(k + 1) % 2] else ins[1:] + ins[0]             # in phase with what follows the anchor: it can move
        recs += [rd(ref, 0, t + k - 6, "7M%dD3M" % n), rd(ref, 0, t + k - 9, "10M%dI4M" % n, ins), rd(ref, 0, t - 1, "%dM%dD1M" % (k + 2, n))]
    return [len(text)], (), ref, recs, at


def test_step_case_crosses_the_steps():
    l_ref, regions, ref, recs, at = step_case()
    pairs = shifts(l_ref, regions, ref, [b"".join(recs)])
    assert len(pairs) == len(recs) and all(a[1] != O for a, _, _ in pairs)
    got = [k for _, _, k in pairs]
    for i, s in enumerate(STEP_SHIFTS):
        assert got[3 * i:3 * i + 3] == [s, s + 1, s] and pairs[3 * i][1][0] == at[s] - 1
    rest = got[3 * len(STEP_SHIFTS):]
    assert rest[:12] == [199, 199, 151, 151, 101, 101, 71, 71, 65, 65, 11, 11]
    ca = rest[12:]
    assert all(k > 0 for k in ca) and max(ca) > 256 and {k // 64 for k in ca} >= {0, 1, 2, 4}
    assert all(b[0] == at["CA300"] - 1 for _, b, _ in pairs[-len(ca):])          # all behind the T before the tract


# Where a shift stops.  Reference 0: A^60 at 30..89 and regions [50, 120) (it begins inside the tract) and [120, 150); a tract T^40
# over 130..169 and the touching regions [120, 150) and [150, 220); A^10 N A^10 at 230..250 in [225, 300).  Reference 1 begins with A^20.
STOP_L_REF, STOP_REGIONS, STOP_NAMES = [320, 60], [(0, 50, 120), (0, 120, 150), (0, 150, 220), (0, 225, 300), (1, 0, 60)], [b"s0", b"s1"]


def stop_case():
    text = "GC" * 15 + "A" * 60 + "GTC" * 13 + "G" + "T" * 40 + "CG" * 30 + "A" * 10 + "N" + "A" * 10 + "CGT" * 23
    ref = [codes(text), codes("A" * 20 + "CGT" * 13 + "C")]
    assert len(text) == 320 and text[130:170] == "T" * 40 and text[129] != "T" and text[240] == "N" and text[29] != "A"
    recs = [rd(ref, 0, 60, "20M1D5M"), rd(ref, 0, 40, "30M2I5M", "AA"), rd(ref, 0, 45, "6M1D30M"),      # to 50; to 50; anchor 50 itself stays
            rd(ref, 0, 40, "8M1D30M"),                                            # anchor 47 has no slot: dropped
            rd(ref, 0, 155, "10M1D10M"), rd(ref, 0, 135, "10M1D10M"), rd(ref, 0, 125, "35M2I3M", "TT"),   # to 150; to 129; to 150
            rd(ref, 0, 245, "3M1D5M"), rd(ref, 0, 228, "8M1D5M"), rd(ref, 0, 226, "20M1I5M", "A"),        # to the N at 240; to 229; to 240
            rd(ref, 1, 0, "10M1D5M"), rd(ref, 1, 0, "15M3I5M", "AAA"), rd(ref, 1, 0, "1M1D5M")]           # to position 0 of reference 1
    return STOP_L_REF, STOP_REGIONS, ref, recs


STOP_PLACES = [(0, 50), (0, 50), (0, 50), (2, 150), (1, 129), (2, 150), (3, 240), (3, 229), (3, 240), (4, 0), (4, 0), (4, 0)]


def test_stop_case_stops_where_it_says():
    l_ref, regions, ref, recs = stop_case()
    p = model(l_ref, regions, ref, [b"".join(recs)])
    assert [p._place(e[0]) for e in p.events] == STOP_PLACES
    assert [k for _, _, k in shifts(l_ref, regions, ref, [b"".join(recs)])] == [29, 19, 0, 14, 15, 9, 7, 6, 5, 9, 14, 0]
    assert [int(c["pos"]) for c in p.indel_calls(0, 1)] == [50, 129, 150, 229, 0]  # none at the N: rule 16


# L = 32, the whole sequence word.  A unit of 32 bases four times over 40..167; its last base differs from the base before the repeat.
L32_L_REF, L32_NAMES = [260], [b"w"]


def l32_case():
    rng = np.random.default_rng(11)
    unit = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, 32))
    assert len({unit[k:] + unit[:k] for k in range(32)}) == 32                    # no shorter period
    pre = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, 40))
    pre = pre[:-1] + "ACGT"[(CODE[unit[-1]] + 1) % 4]
    text = pre + unit * 4 + "".join("ACGT"[int(c)] for c in rng.integers(0, 4, 92))
    ref = [codes(text)]
    rot = lambda k: unit[k % 32:] + unit[:k % 32]
    other = "ACGT"[(CODE[text[120]] + 1) % 4] * 32                                # ends in a base that is not the anchor's: it stays
    recs = [rd(ref, 0, 100, "21M32D20M"), rd(ref, 0, 90, "17M32D10M"),            # anchors 120 and 106: shifts of 81 and 67
            rd(ref, 0, 100, "21M32I20M", rot(121 - 40)), rd(ref, 0, 60, "40M32I5M", rot(100 - 40)),      # anchors 120 and 99: 81 and 60
            rd(ref, 0, 100, "21M32I20M", other), rd(ref, 0, 100, "21M31D20M"), rd(ref, 0, 100, "21M31I20M", rot(121 - 40)[:31]),
            rd(ref, 0, 100, "21M2I20M", "AN"), rd(ref, 0, 100, "21M33D20M")]
    return L32_L_REF, (), ref, recs


def test_l32_case():
    l_ref, regions, ref, recs = l32_case()
    pairs = shifts(l_ref, regions, ref, [b"".join(recs)])
    assert [(a[1], a[2], k) for a, _, k in pairs[:5]] == [(D, 32, 81), (D, 32, 67), (I, 32, 81), (I, 32, 60), (I, 32, 0)]
    assert [(a[1], k) for a, _, k in pairs[7:]] == [(O, 0), (O, 0)] and pairs[5][0][1:3] == (D, 31) and pairs[6][0][1:3] == (I, 31)
    unit = sum(int(c) << (2 * j) for j, c in enumerate(ref[0][40:72]))            # behind the new anchor 39 stands the unit itself
    assert pairs[2][1][3] == pairs[3][1][3] == unit != pairs[2][0][3] and pairs[3][0][3] != unit        # one allele, rotated from what each read gave
    small = shifts(l_ref, regions, ref, [b"".join(recs)], opt={"max_len": 31})
    assert [(a[1], k) for a, _, k in small[:5]] == [(O, 0)] * 5 and small[5][0][1] == D


# Which span a moved event takes back.  A^30 over 20..49 behind a C at 19 (reference 0 of 90).
CLIP_L_REF, CLIP_NAMES = [90], [b"k"]


def clip_case():
    text = "GT" * 9 + "GC" + "A" * 30 + "CGT" * 13 + "C"
    ref = [codes(text)]
    recs = [rd(ref, 0, 35, "5M1D20M"),                     # anchor 39, to 19: the run began at 35, behind the new anchor; its span 35..38 is gone
            rd(ref, 0, 10, "25M1D20M"),                    # anchor 34, to 19: the run began at 10; it keeps 10..18
            rd(ref, 0, 10, "15M8N1D20M"),                  # behind an N op: anchor 32 moves, and clips nothing
            rd(ref, 0, 10, "18M2D1I20M", "A"),             # the D behind 27 moves and clips 19..26; the I behind the D (anchor 29) moves and clips nothing
            rd(ref, 0, 33, "3M2I2D3M", "AA"),              # adjacent: the I clips 33..34 at most ... the D behind the I clips nothing
            rd(ref, 0, 10, "70M"), rd(ref, 0, 38, "4M1P1D9M"), rd(ref, 0, 36, "2M2=1X1D9M")]      # behind a P: nothing; M = X are one run
    return CLIP_L_REF, (), ref, recs


def test_clip_case():
    l_ref, regions, ref, recs = clip_case()
    on = model(l_ref, regions, ref, [b"".join(recs)])
    off = model(l_ref, regions, ref, [b"".join(recs)], False)
    assert all(p == (0, 19) for p in (on._place(e[0]) for e in on.events)) and len(on.events) == 9
    lost = (off.span - on.span)[:, 0].tolist()
    want = [0] * 90
    for lo, hi in ((35, 39), (19, 34), (19, 27), (33, 35), (36, 40)):              # per record, the slots its clipped run lost
        for s in range(lo, hi):
            want[s] += 1
    assert lost == want and (on.span >= 0).all()
    assert on.span[19:27, 0].tolist() == [2] * 5 + [1] * 3                         # the 70M read, and to 23 the 15M before the N skip


# One add of 301 records with every kind in every wave, then a second add of 150.
MIX_L_REF, MIX_REGIONS, MIX_NAMES = [1400], [(0, 0, 700), (0, 700, 1400)], [b"m"]


def mix_case():
    rng = np.random.default_rng(17)
    text = ("GC" + "A" * 150 + "TG" + _tract("CA", 180) + "GGT" + _tract("ACG", 90) + "T" + "".join("ACGT"[int(c)] for c in rng.integers(0, 4, 272)))
    text += text[::-1]
    ref = [codes(text)]
    assert len(text) == 1400
    recs = []
    for k in range(451):
        kind = k % 7
        if kind == 0:
            recs.append(rd(ref, 0, int(rng.integers(0, 1300)), "60M", mapq=int(rng.choice([3, 30, 60]))))        # no event
        elif kind == 1:
            recs.append(rd(ref, 0, int(rng.integers(430, 650)), "12M1D12M"))                                    # mostly unmoved
        elif kind == 2:
            recs.append(rd(ref, 0, int(rng.integers(0, 8)), "%dM1D4M" % int(rng.integers(10, 22))))             # short shifts in A^150
        elif kind == 3:
            recs.append(rd(ref, 0, 0, "%dM2D4M" % int(rng.integers(80, 150)), mapq=int(rng.choice([20, 60]))))   # over 64
        elif kind == 4:
            a = int(rng.integers(160, 320))
            recs.append(rd(ref, 0, a - 10, "11M2I6M", "".join("ACGT"[int(c)] for c in ref[0][a + 1:a + 3])))     # (CA)n, any phase
        elif kind == 5:
            a = int(rng.integers(760, 1060))
            recs.append(rd(ref, 0, a - 7, "8M3D6M", flag=int(rng.choice([0, 16, 0x400]))))                       # the mirror half, its own region
        else:
            recs.append(rd(ref, 0, int(rng.integers(100, 140)), "9M40I9M", "A" * 40))                           # OTHER: too long
    return MIX_L_REF, MIX_REGIONS, ref, [recs[:301], recs[301:]]


def test_mix_case():
    l_ref, regions, ref, adds = mix_case()
    pairs = shifts(l_ref, regions, ref, [b"".join(a) for a in adds])
    ks = [k for _, _, k in pairs]
    assert sum(k == 0 for k in ks) > 60 and sum(0 < k <= 8 for k in ks) > 20 and sum(k > 64 for k in ks) > 60
    assert any(a[1] == O for a, _, _ in pairs) and len(adds[0]) % 64 != 0
    p = model(l_ref, regions, ref, [b"".join(a) for a in adds])
    assert (p.span >= 0).all() and len(p.indel_calls(0, 1)) >= 5
