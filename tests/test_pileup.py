"""The pileup rules (include/bwams.h above bwams_pileup_open) on hand-built records: bwams/pileup.py against counters, sites and
texts written out here, and against planted truth.  tests/test_gpu_pileup.py runs the same records through the C-ABI."""
import struct

import numpy as np
import pytest

from bwams import bam, pileup, simulate
from test_depth import OPS

CH = {name: k for k, name in enumerate(pileup.CHANNELS)}


def prec(refid: int, pos: int, cigar, seq, qual=30, flag: int = 0, mapq: int = 60, name: bytes = b"r") -> bytes:
    """One BAM record with real SEQ nibbles.  cigar: text ("3M2D3M"; "" for none) or a list of (length, op code).  seq: letters of
    "=ACMGRSVTWYHKDBN" or a code array (0..15), "" for SEQ `*`.  qual: one value for every base, a list per base, or None for absent
    qualities (0xFF bytes)."""
    if isinstance(cigar, str):
        ops, n = [], ""
        for ch in cigar:
            if ch.isdigit():
                n += ch
            else:
                ops.append((int(n), OPS[ch]))
                n = ""
    else:
        ops = list(cigar)
    codes = [bam.NT16.index(c) for c in seq.encode()] if isinstance(seq, str) else [int(c) for c in seq]
    l_seq = len(codes)
    quals = [0xFF] * l_seq if qual is None else [qual] * l_seq if isinstance(qual, int) else list(qual)
    assert len(quals) == l_seq
    rlen = sum(n for n, op in ops if op in (0, 2, 3, 7, 8))
    end = pos + rlen if rlen and not flag & 4 else pos + 1
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(name) + 1, mapq, bam.reg2bin(max(pos, 0), max(end, 1)) & 0xFFFF, len(ops), flag, l_seq,
                       -1, -1, 0)
    body += name + b"\0" + b"".join(struct.pack("<I", n << 4 | op) for n, op in ops)
    padded = codes + [0] * (l_seq & 1)
    body += bytes(padded[k] << 4 | padded[k + 1] for k in range(0, l_seq, 2)) + bytes(quals)
    return struct.pack("<I", len(body)) + body


def ch(*names):
    """a slot with 1 in each named channel (a name may repeat)"""
    out = [0] * 12
    for n in names:
        out[CH[n]] += 1
    return out


# One reference of 20 bases, one of 6; regions: [2, 12) and [12, 16) of reference 0 (touching), [1, 2) of reference 1 (one position).
L_REF = [20, 6]
REGIONS = [(0, 2, 12), (0, 12, 16), (1, 1, 2)]
NAMES = [b"c0", b"c1"]
HAND = [
    prec(0, 0, "6M", "ACGTAC"),                                   # 0  positions 0 1 outside every region; 2..5 = G T A C forward
    prec(0, 3, "3M", "TTA", flag=0x10),                           # 1  reverse strand: T- T- A- at 3 4 5
    prec(0, 4, "2M2D2M", "AAGG"),                                 # 2  A A at 4 5, DEL at 6 7, G G at 8 9
    prec(0, 5, "2S1M2I1M1P1I2M", "NNCTTGAAC"),                    # 3  C at 5, INS at 5, G at 6, INS at 6 (behind the P), A C at 7 8
    prec(0, 2, "2I3M", "TTGTA"),                                  # 4  an insertion that opens the alignment: not counted; G T A at 2 3 4
    prec(0, 9, "1M3N2M", "ARN"),                                  # 5  A at 9, the skip counts nothing, R (code 5) and N -> N at 13 14
    prec(0, 10, "3=1X", "=A=C"),                                  # 6  code 0 at 10 -> N, A at 11, code 0 at 12 -> N, C at 13 (region 1)
    prec(0, 14, "4M", "ACGT", qual=[13, 12, 13, 12]),             # 7  quality 13 counts, 12 does not: A at 14, G at 16 (outside)
    prec(0, 15, "3M", "CCC", qual=None),                          # 8  no qualities: all pass; C at 15, 16 17 outside
    prec(0, 10, "1M4D1M", "AC", qual=[0, 40]),                    # 9  A fails its quality; DEL at 11 | 12 13 14 (across the regions' edge); C at 15
    prec(0, 18, "5M", "AAAAA"),                                   # 10 runs off the reference's end, and outside every region
    prec(0, 25, "3M", "AAA"),                                     # 11 POS past the end: counts, adds nothing
    prec(1, 0, "3M", "ACG"),                                      # 12 only position 1 is a slot: C
    prec(1, 1, "1M1I", "TT", flag=0x10),                          # 13 T- at 1, INS at 1
    prec(1, -1, [(3, 0)], "GGG"),                                 # 14 POS below 0: position -1 dropped, G at 1 (0 is outside)
    prec(0, 0, "10M", "AAAAAAAAAA", flag=0x400),                  # skipped: duplicate
    prec(0, 6, "2M", "TT", flag=0x800),                           # 15 supplementary: counts; T T at 6 7
    prec(-1, 0, "5M", "AAAAA"), prec(2, 0, "5M", "AAAAA"), prec(0, 3, "", "AAA"), prec(0, 3, "5M", ""),      # skipped: no reference,
]                                                                 # refID == n_ref, no CIGAR, l_seq 0
N_COUNTED = 16
WANT = [
    [ch("G+", "G+"), ch("T+", "T-", "T+"), ch("A+", "T-", "A+", "A+"), ch("C+", "A-", "A+", "C+", "INS"), ch("DEL", "G+", "INS", "T+"),
     ch("DEL", "A+", "T+"), ch("G+", "C+"), ch("G+", "A+"), ch("N"), ch("A+", "DEL")],                       # positions 2 .. 11
    [ch("N", "DEL"), ch("N", "C+", "DEL"), ch("N", "A+", "DEL"), ch("C+", "C+")],                           # positions 12 .. 15
    [ch("C+", "T-", "INS", "G+")],                                                                           # reference 1, position 1
]
# reference bases for the sites: reference 0 = ACGTACGTACGTACGTACGT, and C at position 1 of reference 1
REF0 = np.array([0, 1, 2, 3] * 5, np.uint8)


def hand(**kw) -> pileup.Pileup:
    p = pileup.Pileup(L_REF, REGIONS, **kw)
    assert p.add(b"".join(HAND)) == N_COUNTED
    return p


def test_hand_counters():
    p = hand()
    assert [p.fetch(k).tolist() for k in range(3)] == WANT
    assert p.fetch(0, 4, 6).tolist() == WANT[0][2:4] and p.fetch(1, 13, 13).tolist() == []
    p.reset()
    assert not p.c.any()
    for part in (HAND[11:], HAND[:5], HAND[5:11]):                 # any order, any number of calls
        p.add(b"".join(part))
    assert [p.fetch(k).tolist() for k in range(3)] == WANT


# an I behind S only has no reference op before it and is not counted; an I behind a D is, at the last deleted position; two I
# around a P share the anchor of the M before them (every I op adds 1, P does nothing), between H clips that do nothing either
INS_RECS = [prec(0, 4, "2S1I2M", "NNTAC"), prec(0, 4, "1M1D1I1M", "ATC"), prec(0, 4, "2H1M1I1P1I2M3H", "GTTAC")]
INS_WANT = [ch("A+", "A+", "G+", "INS", "INS"), ch("C+", "DEL", "INS", "A+"), ch("C+", "C+")]        # positions 4 5 6


def test_insertions():
    p = pileup.Pileup([10])
    assert p.add(b"".join(INS_RECS)) == 3 and p.fetch(0, 4, 7).tolist() == INS_WANT and not p.fetch(0, 0, 4).any()


def test_hand_sites():
    p = hand(min_alt=1, min_permille=300)
    assert not len(p.sites())                                      # before set_ref every base is 4: no site
    p.set_ref(0, REF0[2:12])
    p.set_ref(1, REF0[12:16])
    p.set_ref(2, [1])
    s = p.sites()
    # position 5 (ref C): depth 4 = C+ A- A+ C+; A has 2 (500 permille), INS 1 (250: out).  6 (ref G): DEL 1 of 3, T 1 of 3, INS 1 of 3.
    # 7 (T): DEL 1 of 3, A 1 of 3.  8 (A): G 1 of 2, C 1 of 2.  9 (C): G 1 of 2, A 1 of 2.  11 (T): depth 2 = A+ DEL.  12 (A): depth 1 = DEL.
    # 13 (C): depth 2 = C+ DEL.  14 (G): depth 2 = A+ DEL.  15 (T): C 2 of 2.  reference 1 position 1 (C): depth 3, T 1, G 1, INS 1.
    # Not sites: 2 3 (reference only), 4 (T- 1 of 4 is 250 permille), 10 (N only: depth 0, no allele has a count).
    want = [(0, 5, 1, 0b000001, 4), (0, 6, 2, 0b111000, 3), (0, 7, 3, 0b010001, 3), (0, 8, 0, 0b000110, 2), (0, 9, 1, 0b000101, 2),
            (0, 11, 3, 0b010001, 2), (1, 12, 0, 0b010000, 1), (1, 13, 1, 0b010000, 2), (1, 14, 2, 0b010001, 2), (1, 15, 3, 0b000010, 2),
            (2, 1, 1, 0b101100, 3)]
    assert [(int(x["region"]), int(x["pos"]), int(x["ref"]), int(x["kinds"]), int(x["depth"])) for x in s] == want
    assert s["c"][0].tolist() == WANT[0][3] and s["c"][-1].tolist() == WANT[2][0]
    assert [int(x["pos"]) for x in p.sites(2, 0)] == [5, 15]       # two of one alternate allele: A at 5, C at 15
    p.set_ref(1, [4, 4, 4, 4])                                     # an N in the reference is no site
    assert [int(x["region"]) for x in p.sites()] == [0] * 6 + [2]


def test_filters_and_refusals():
    data = prec(0, 2, "3M", "AAA", mapq=29) + prec(0, 2, "3M", "CCC", mapq=30) + prec(0, 2, "3M", "GGG", flag=0x100)
    p = pileup.Pileup([10], min_mapq=30)
    assert p.add(data) == 1 and p.fetch(0, 2, 3).tolist() == [ch("C+")]
    p = pileup.Pileup([10], exclude=0)
    assert p.add(data) == 3 and p.fetch(0, 2, 3).tolist() == [ch("A+", "C+", "G+")]
    p = pileup.Pileup([10], min_baseq=0)
    assert p.add(prec(0, 0, "2M", "AC", qual=[0, 1])) == 1 and p.fetch(0, 0, 2).tolist() == [ch("A+"), ch("C+")]
    p = pileup.Pileup([10])
    p.add(prec(0, 0, "3M", "AAA"))
    with pytest.raises(pileup.PileupRefusal) as e:                 # an op code above 8, counted or not; nothing of the call is added
        p.add(prec(0, 0, "2M", "CC") + prec(-1, 0, [(2, 0), (1, 9)], "CC", flag=0x4) + prec(0, 0, [(1, 12)], "C"))
    assert (e.value.record, e.value.why) == (1, "op")
    with pytest.raises(pileup.PileupRefusal) as e:                 # the query length, only of a record the filter lets through
        p.add(prec(0, 0, "2M", "CCC", flag=0x400) + prec(0, 0, "2M1I", "CC") + prec(0, 0, "2M", "CCC"))
    assert (e.value.record, e.value.why) == (1, "length")
    short = bytearray(prec(0, 0, "9M", "ACGTACGTA")[:-3])                    # QUAL ends behind the record: refused when it counts
    short[0:4] = (len(short) - 4).to_bytes(4, "little")
    with pytest.raises(pileup.PileupRefusal) as e:
        p.add(prec(0, 0, "2M", "CC") + bytes(short))
    assert (e.value.record, e.value.why) == (1, "bounds")
    short[18:20] = (0x400).to_bytes(2, "little")
    assert p.add(bytes(short)) == 0
    assert p.fetch(0, 0, 4).tolist() == [ch("A+")] * 3 + [ch()]
    for bad in ([(0, 5, 5)], [(0, 0, 11)], [(1, 0, 1)], [(0, 0, 5), (0, 4, 8)], [(0, 5, 8), (0, 0, 5)], [(0, -1, 3)]):
        with pytest.raises(AssertionError):
            pileup.Pileup([10], bad)
    assert pileup.Pileup([10, 0, 7]).regions == [(0, 0, 10), (2, 0, 7)]


# the worked example of include/bwams.h's rule 9
EX_L_REF, EX_NAMES, EX_REF = [8], [b"c1"], [0, 1, 2, 3, 0, 1, 2, 3]
EX_RECS = [prec(0, 0, "8M", "ACGTACGT"), prec(0, 0, "8M", "ACTTACGT"), prec(0, 0, "8M", "ACTTACGT", flag=0x10),
           prec(0, 2, "2M1D2M", "GTCG"), prec(0, 2, "2M1D2M", "GTCG"), prec(0, 4, "2M2I2M", "ACTTGT"), prec(0, 4, "2M2I2M", "ACTTGT")]
EX_TEXT = ("chrom\tpos\tref\tdepth\tA+\tC+\tG+\tT+\tA-\tC-\tG-\tT-\tN\tDEL\tINS\talt\n"
           "c1\t3\tG\t5\t0\t0\t3\t1\t0\t0\t0\t1\t0\t0\t0\tT\n" "c1\t5\tA\t7\t4\t0\t0\t0\t1\t0\t0\t0\t0\t2\t0\tDEL\n"
           "c1\t6\tC\t7\t0\t6\t0\t0\t0\t1\t0\t0\t0\t0\t2\tINS\n")
HAND_TEXT = (pileup.TEXT_HEADER + "c0\t6\tC\t4\t1\t2\t0\t0\t1\t0\t0\t0\t0\t0\t1\tA\n" "c0\t7\tG\t3\t0\t0\t1\t1\t0\t0\t0\t0\t0\t1\t1\tT,DEL,INS\n")


def example() -> pileup.Pileup:
    p = pileup.Pileup(EX_L_REF)
    assert p.add(b"".join(EX_RECS)) == 7
    p.set_ref(0, EX_REF)
    return p


def test_texts():
    assert example().text(EX_NAMES) == EX_TEXT
    p = hand(min_alt=1, min_permille=300)
    p.set_ref(0, REF0[2:12])
    assert p.text(NAMES).startswith(HAND_TEXT) and p.text(NAMES).count("\n") == 7
    assert pileup.Pileup([5]).text([b"x"]) == pileup.TEXT_HEADER


def planted(seed: int = 7):
    """a 20 kb genome, 40 SNVs at least 200 bp apart, error-free 100 bp reads every 10 bp on both strands"""
    rng = np.random.default_rng(seed)
    ref = simulate.make_genome(20000, seed=seed, repeat_frac=0.0)
    at = np.sort(rng.choice(np.arange(0, 20000, 250), 40, replace=False) + rng.integers(0, 50, 40))
    sample = ref.copy()
    sample[at] = (ref[at] + rng.integers(1, 4, 40)) % 4
    recs = []
    for k, pos in enumerate(range(0, 20000 - 100 + 1, 10)):
        fw = sample[pos:pos + 100]
        for rev in (0, 1):                                         # BAM holds the forward-strand bases of either strand's read
            recs.append(prec(0, pos, "100M", [1 << int(c) for c in fw], flag=0x10 * rev, name=b"t%d" % k))
    return ref, sample, at, recs


def test_planted_truth():
    ref, sample, at, recs = planted()
    assert len(at) == 40 and (np.diff(at) >= 200).all()
    p = pileup.Pileup([20000])
    assert p.add(b"".join(recs)) == len(recs)
    p.set_ref(0, ref)
    s = p.sites()
    covered = [int(x) for x in at if p.c[x, :8].sum() >= 2]
    assert len(covered) == 40                                      # every position has two reads at least: 20 on either strand inside
    assert [int(x) for x in s["pos"]] == covered                   # every planted position, and no other
    for x in s:
        assert int(x["kinds"]) == 1 << int(sample[int(x["pos"])]) and int(x["ref"]) == int(ref[int(x["pos"])])
        assert int(x["c"][int(sample[int(x["pos"])])]) == int(x["c"][int(sample[int(x["pos"])]) + 4]) == int(x["depth"]) // 2


def test_prec_matches_the_sam_encoder():
    line = b"\t".join([b"r", b"16", b"c0", b"5", b"37", b"2S3M1I2M", b"*", b"0", b"0", b"ACGTNACG", b"IIIIIII5"])
    assert prec(0, 4, "2S3M1I2M", "ACGTNACG", qual=[40] * 7 + [20], flag=16, mapq=37) == bam.encode_record(line, {b"c0": 0})
    f = pileup.fields(prec(3, 7, "4M2D", "ACGT", qual=[1, 2, 3, 4], flag=99, mapq=5))
    assert f[:4] == (3, 7, 5, 99) and f[5] == 4 and f[6].tolist() == [1, 2, 4, 8] and f[7].tolist() == [1, 2, 3, 4]
    assert pileup.fields(prec(0, 0, "3M", "ACG"))[6].tolist() == [1, 2, 4]          # odd l_seq: the last nibble is padding
