"""Duplicate marking's rules (include/bwams.h above bwams_bam_templates) on hand-built records: bwams/markdup.py against flags and
counts written out here.  tests/test_gpu_markdup.py runs the same cases through bwams_bam_upload + bwams_bam_markdup."""
import re
import struct

import pytest

from bwams import bam, markdup

D = 0x400
REF_ID = {b"c0": 0, b"c1": 1}


def qlen(cigar: bytes) -> int:
    return sum(int(n) for n, op in re.findall(rb"([0-9]+)([MIS=X])", cigar))


def rec(name: bytes, flag: int, pos0: int, cigar: bytes = b"50M", qual: bytes | None = b"I", ref: bytes = b"c0") -> bytes:
    """one record: qual is one character repeated over the read, or None for QUAL '*'"""
    n = qlen(cigar) if cigar != b"*" else 10
    q = b"*" if qual is None else qual * n
    line = b"\t".join([name, b"%d" % flag, ref, b"%d" % (pos0 + 1), b"60", cigar, b"*", b"0", b"0", b"A" * n, q])
    return bam.encode_record(line, REF_ID)


P1, P2 = 0x1 | 0x40, 0x1 | 0x80                          # paired: first, last
R = 0x10

# (case, records, the FLAG 0x400 each record must end up with, counts)
CASES = [
    ("clips_forward", [rec(b"a", 0, 100, b"50M", b"I"),               # unclipped 100, score 50 * 40
                       rec(b"b", 0, 103, b"3S47M", b"5"),             # 103 - 3 = 100, score 50 * 20
                       rec(b"c", 0, 105, b"2H3S45M", b"5"),           # 105 - 5 = 100, score 48 * 20
                       rec(b"d", 0, 101, b"50M", b"5")],              # 101: a group of its own
     [0, D, D, 0], dict(templates=4, unpaired_examined=4, unpaired_duplicates=2, pairs_examined=0, pair_duplicates=0, records_marked=2)),
    ("clips_reverse", [rec(b"e", R, 200, b"40M10S", b"I"),            # 200 + 40 - 1 + 10 = 249, score 2000
                       rec(b"f", R, 200, b"50M", b"5"),               # 249, score 1000
                       rec(b"g", R, 205, b"20M5D15M5H", b"I"),        # rlen 40: 205 + 40 - 1 + 5 = 249, score 1400
                       rec(b"h", 0, 249, b"50M", b"I")],              # forward at 249: another strand
     [0, D, D, 0], dict(templates=4, unpaired_examined=4, unpaired_duplicates=2, pairs_examined=0, pair_duplicates=0, records_marked=2)),
    ("fr_rf", [rec(b"p1", P1, 300), rec(b"p1", P2 | R, 500),           # FR: (300 +, 549 -)
               rec(b"p2", P1 | R, 251), rec(b"p2", P2, 549),           # RF: (300 -, 549 +)
               rec(b"p3", P2 | R, 500, qual=b"5"), rec(b"p3", P1, 300, qual=b"5")],   # FR again, last end first, lower score
     [0, 0, 0, 0, D, D], dict(templates=3, unpaired_examined=0, unpaired_duplicates=0, pairs_examined=3, pair_duplicates=1, records_marked=2)),
    ("ties_earlier", [rec(b"t1", 0, 400), rec(b"t2", 0, 400), rec(b"u1", P1, 450), rec(b"u1", P2 | R, 700),
                      rec(b"u2", P2 | R, 700), rec(b"u2", P1, 450)],
     [0, D, 0, 0, D, D], dict(templates=4, unpaired_examined=2, unpaired_duplicates=1, pairs_examined=2, pair_duplicates=1, records_marked=3)),
    ("score_cap", [rec(b"cap1", 0, 1000, b"450M"),                     # 450 * 40 = 18000 -> 16383
                   rec(b"cap2", 0, 1000, b"500M")],                    # 20000 -> 16383: a tie, the earlier kept
     [0, D], dict(templates=2, unpaired_examined=2, unpaired_duplicates=1, pairs_examined=0, pair_duplicates=0, records_marked=1)),
    ("qual_absent", [rec(b"q1", 0, 1200, qual=None),                   # score 0 (not 50 * 0xFF)
                     rec(b"q2", 0, 1200, qual=b"0"),                   # 50 * 15
                     rec(b"q3", 0, 1300, qual=b"."),                   # 50 * 13: below 15, score 0
                     rec(b"q4", 0, 1300, qual=b"/")],                  # 50 * 14: score 0, a tie
     [D, 0, 0, D], dict(templates=4, unpaired_examined=4, unpaired_duplicates=2, pairs_examined=0, pair_duplicates=0, records_marked=2)),
    ("fragment_vs_pair_end", [rec(b"fp", P1, 600, qual=b"#"), rec(b"fp", P2 | R, 800, qual=b"#"),
                              rec(b"fx", P1 | 0x8, 600), rec(b"fx", P2 | 0x4, 600, b"*")],    # a fragment with its mate unmapped
     [0, 0, D, D], dict(templates=2, unpaired_examined=1, unpaired_duplicates=1, pairs_examined=1, pair_duplicates=0, records_marked=2)),
    ("two_fragments", [rec(b"x1", R, 900, qual=b"5"), rec(b"x2", R, 900, qual=b"I")],
     [D, 0], dict(templates=2, unpaired_examined=2, unpaired_duplicates=1, pairs_examined=0, pair_duplicates=0, records_marked=1)),
    ("secondary_supplementary_unmapped", [
        rec(b"sk", 0, 1500),
        rec(b"sd", P1 | 0x8, 1500, qual=b"5"), rec(b"sd", P1 | 0x8 | 0x800, 3000, b"30H20M", b"5", ref=b"c1"),
        rec(b"sd", P1 | 0x8 | 0x100, 4000, b"50M", b"5"), rec(b"sd", P2 | 0x4, 1500, b"*"),
        rec(b"none", 0x4, -1, b"*", ref=b"*")],                          # no mapped primary: never a duplicate
     [0, D, D, D, D, 0], dict(templates=3, unpaired_examined=2, unpaired_duplicates=1, pairs_examined=0, pair_duplicates=0, records_marked=4)),
    ("stale_cleared", [rec(b"s1", D, 2000), rec(b"s2", D | R, 2000), rec(b"s3", 0, 2000, qual=b"5")],
     [0, 0, D], dict(templates=3, unpaired_examined=3, unpaired_duplicates=1, pairs_examined=0, pair_duplicates=0, records_marked=1)),
]

FAR = (1 << 31) - 100


def far(r: bytes) -> bytes:                             # POS near 2^31 has no bin that fits 16 bits: patched in after encoding
    return r[:8] + struct.pack("<i", FAR) + r[12:]


# (case, records, the first record concerned, reason: index into markdup.REASONS)
REFUSALS = [
    ("two_only", [rec(b"a", 0, 10), rec(b"r", 0, 20), rec(b"r", 0, 30)], 2, 0),
    ("two_first", [rec(b"r", P1, 10), rec(b"r", P1, 20), rec(b"r", P2, 30)], 1, 0),
    ("neither_bit", [rec(b"r", P1, 10), rec(b"r", 0x1, 20)], 1, 1),
    ("both_bits", [rec(b"r", 0x1 | 0x40 | 0x80, 10)], 0, 1),
    ("mixed", [rec(b"r", P1, 10), rec(b"r", 0x100, 15), rec(b"r", 0, 20)], 2, 2),
    ("coordinate_low", [rec(b"a", 0, 5, b"268435455H" * 9 + b"50M")], 0, 3),
    ("coordinate_high", [rec(b"a", 0, 5), far(rec(b"b", R, 0, b"50M200S"))], 1, 3),
    ("refid_unplaced", [rec(b"a", 0, 5, ref=b"*")], 0, 3),
    ("first_of_several", [rec(b"ok", 0, 10), rec(b"m", 0, 20), rec(b"m", 0x1 | 0x40, 20),
                          rec(b"d", 0, 10), rec(b"d", 0, 10)], 2, 2),
]


def flags(records: bytes) -> list[int]:
    return [struct.unpack_from("<H", r, 18)[0] for r in bam.split_records(records)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_rules(case):
    _, recs, want, counts = case
    (out,), got = markdup.mark([b"".join(recs)])
    assert [f & D for f in flags(out)] == want
    assert [f & ~D for f in flags(out)] == [f & ~D for f in flags(b"".join(recs))]            # nothing but 0x400 changes
    assert {k: got[k] for k in counts} == counts
    assert bam.split_records(out) != [] and len(out) == len(b"".join(recs))


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals(case):
    _, recs, at, why = case
    with pytest.raises(markdup.MarkdupRefusal) as e:
        markdup.mark([b"".join(recs)])
    assert (e.value.record, e.value.reason) == (at, why)


def test_ends_and_templates():
    recs = [rec(b"p", P2 | R, 500, b"45M5S"), rec(b"p", P1, 300, b"2S48M"), rec(b"p", P1 | 0x800, 900, b"20M30H"),
            rec(b"q", 0x4, -1, b"*", ref=b"*"), rec(b"s", R, 40, b"10M", b"*")]
    assert markdup.templates(recs) == [(0, 3), (3, 4), (4, 5)]
    n_t, es, rt = markdup.ends(recs)
    assert n_t == 3 and rt == [0, 0, 0, 1, 2]
    assert es == [dict(tmpl=0, ref1=0, pos1=298, ref2=0, pos2=549, score=2000 + 2000, strands=0b10),   # end 1: the smaller coordinate
                  dict(tmpl=2, ref1=0, pos1=49, ref2=-1, pos2=0, score=0, strands=1)]


def test_across_runs_seq_order_and_percent():
    a = [rec(b"a", 0, 100, qual=b"5")]
    b = [rec(b"b", 0, 100, qual=b"5"), rec(b"c", P1, 100), rec(b"c", P2 | R, 300)]
    (ra, rb), st = markdup.mark([b"".join(a), b"".join(b)])
    assert [f & D for f in flags(ra) + flags(rb)] == [D, D, 0, 0]       # a pair end at 100: both fragments marked
    assert st["percent_duplication"] == pytest.approx(2 / 4)
    (rb2, ra2), _ = markdup.mark([b"".join(b[:1]), b"".join(a)])
    assert [f & D for f in flags(rb2) + flags(ra2)] == [0, D]           # a tie: the earlier put wins


def test_decide_direct():
    es = [dict(tmpl=2, ref1=0, pos1=5, ref2=-1, pos2=0, score=10, strands=0),
          dict(tmpl=0, ref1=0, pos1=5, ref2=-1, pos2=0, score=10, strands=0),
          dict(tmpl=1, ref1=0, pos1=5, ref2=-1, pos2=0, score=11, strands=1)]
    dup, st = markdup.decide(es, 4)
    assert dup == [False, False, True, False] and st["unpaired_duplicates"] == 1
