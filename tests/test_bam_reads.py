"""bwams/bam_reads.py, the restatement of `samtools fastq` in front of `bwa mem` (rules 1-7 of include/bwams.h above
bwams_bam_reads_decode), against hand-built records: one case per rule.  No GPU."""
import struct

import numpy as np
import pytest

from bwams import bam_reads
from bam_reads_util import NT16, rand_qual, rand_seq, read_of, rec, same_reads


def test_forward_and_reverse():
    q = b"!#5?I"
    recs = rec(b"fwd", 0, b"ACGTN", q) + rec(b"rev", 0x10, b"AACGN", q)
    got = bam_reads.reads(recs)
    same_reads(got, [read_of(b"fwd", 0, b"ACGTN", q), read_of(b"rev", 0x10, b"AACGN", q)])
    assert list(got[1][1]) == [4, 1, 2, 3, 3] and got[1][2] == b"I?5#!"


def test_all_nibble_codes_in_both_orientations():
    q = bytes(range(40, 56))
    got = bam_reads.reads(rec(b"a", 0, NT16, q) + rec(b"b", 0x10, NT16, q))
    fwd = [4, 0, 1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4]                 # codes 1, 2, 4, 8 are A, C, G, T
    assert list(got[0][1]) == fwd
    assert list(got[1][1]) == [3 - c if c < 4 else 4 for c in fwd[::-1]]
    assert got[0][2] == q and got[1][2] == q[::-1]


@pytest.mark.parametrize("l_seq", [1, 2, 3, 151])
@pytest.mark.parametrize("flag", [0, 0x10])
def test_lengths_that_end_on_a_half_byte(l_seq, flag):
    rng = np.random.default_rng(l_seq)
    s, q = rand_seq(rng, l_seq), rand_qual(rng, l_seq)
    recs = rec(b"x", flag, s, q) + rec(b"y", flag ^ 0x10, s, q)
    same_reads(bam_reads.reads(recs), [read_of(b"x", flag, s, q), read_of(b"y", flag ^ 0x10, s, q)])
    assert bam_reads.count(recs) == (2, 2, 2 * l_seq)


def test_secondary_and_supplementary_records_are_skipped():
    rng = np.random.default_rng(1)
    flags = [0x100, 0x800, 0, 0x110, 0x900, 0x10, 0, 0x800, 0x100]
    seqs = [rand_seq(rng, 20 + k) for k in range(len(flags))]
    quals = [rand_qual(rng, 20 + k) for k in range(len(flags))]
    recs = b"".join(rec(b"n%d" % k, f, seqs[k], quals[k]) for k, f in enumerate(flags))
    want = [read_of(b"n%d" % k, f, seqs[k], quals[k]) for k, f in enumerate(flags) if not f & 0x900]
    same_reads(bam_reads.reads(recs), want)
    assert bam_reads.count(recs) == (9, 3, 22 + 25 + 26)
    # a skipped record may be anything inside: no bases, no qualities, a float tag
    same_reads(bam_reads.reads(rec(b"s", 0x100, b"", None, [b"XF:f:1.5"]) + recs, b"XF"), want)
    assert bam_reads.reads(rec(b"s", 0x100) + rec(b"t", 0x800)) == []
    assert bam_reads.reads(b"") == []


def test_no_qualities_anywhere_and_mixed():
    a, b = rec(b"a", 0, b"ACGT", None), rec(b"b", 0x10, b"AAC", None)
    got = bam_reads.reads(a + b)
    assert [g[2] for g in got] == [None, None]
    assert bam_reads.to_fastq(a + b) == b">a\nACGT\n>b\nGTT\n"
    with pytest.raises(bam_reads.Unsupported) as e:
        bam_reads.reads(a + rec(b"skipped", 0x100, b"AC", b"II") + b + rec(b"c", 0, b"AC", b"II"))
    assert e.value.ordinal == 3 and e.value.offset == len(a) + len(rec(b"skipped", 0x100, b"AC", b"II")) + len(b)
    with pytest.raises(bam_reads.Unsupported) as e:
        bam_reads.reads(rec(b"c", 0, b"AC", b"II") + a)
    assert e.value.ordinal == 1


def test_a_read_without_bases_is_refused():
    with pytest.raises(bam_reads.Unsupported) as e:
        bam_reads.reads(rec(b"a", 0, b"AC", b"II") + rec(b"empty", 0, b"", None))
    assert e.value.ordinal == 1


def test_tags_follow_the_list_not_the_record():
    r = rec(b"a", 0, b"ACGT", b"IIII", [b"BC:Z:ACGT", b"RG:Z:grp", b"XA:A:q", b"XH:H:1AE3", b"RG:Z:second"])
    assert bam_reads.reads(r, b"RGBC")[0][3] == b"RG:Z:grp\tBC:Z:ACGT"
    assert bam_reads.reads(r, b"BCRG")[0][3] == b"BC:Z:ACGT\tRG:Z:grp"
    assert bam_reads.reads(r, b"XHZZXA")[0][3] == b"XH:H:1AE3\tXA:A:q"
    assert bam_reads.reads(r, b"ZZ")[0][3] == b"" and bam_reads.reads(r)[0][3] == b""
    assert bam_reads.to_fastq(r, b"RGXA") == b"@a RG:Z:grp\tXA:A:q\nACGT\n+\nIIII\n"
    with pytest.raises(ValueError):
        bam_reads.reads(r, b"RGB")
    with pytest.raises(ValueError):
        bam_reads.reads(r, b"AB" * 33)


def test_every_integer_width():
    vals = [-128, 255, -32768, 65535, -(1 << 31), (1 << 32) - 1, 0, -1]      # c C s S i I C c
    aux = [b"X%d:i:%d" % (k, v) for k, v in enumerate(vals)]
    r = rec(b"a", 0, b"AC", b"II", aux)
    types = [r[p + 2:p + 3] for p in range(len(r)) if r[p:p + 1] == b"X" and r[p + 1:p + 2].isdigit()]
    assert types == [b"c", b"C", b"s", b"S", b"i", b"I", b"C", b"c"]
    assert bam_reads.reads(r, b"".join(b"X%d" % k for k in range(8)))[0][3] == b"\t".join(aux)


def test_float_and_array_tags():
    f = rec(b"a", 0, b"AC", b"II", [b"XF:f:2.5", b"RG:Z:g"])
    assert bam_reads.reads(f, b"RG")[0][3] == b"RG:Z:g"                   # not listed: walked over
    with pytest.raises(bam_reads.Unsupported):
        bam_reads.reads(f, b"RGXF")
    arr = b"XBBs" + struct.pack("<I", 3) + struct.pack("<3h", 1, -2, 3)
    g = rec(b"a", 0, b"AC", b"II", [b"RG:Z:g"], raw_aux=arr + b"NMC\x07")
    assert bam_reads.reads(g, b"NMRG")[0][3] == b"NM:i:7\tRG:Z:g"
    with pytest.raises(bam_reads.Unsupported):
        bam_reads.reads(g, b"XB")
    # only a tag's first field counts
    assert bam_reads.reads(rec(b"a", 0, b"AC", b"II", [b"XF:i:3", b"XF:f:2.5"]), b"XF")[0][3] == b"XF:i:3"


def test_malformed_aux_fields():
    cut = rec(b"a", 0, b"AC", b"II", raw_aux=b"RGZabc")                    # no NUL inside the record
    assert bam_reads.reads(cut)[0][0] == b"a"                             # no tags listed: the aux fields are not walked
    for bad in (cut, rec(b"a", 0, b"AC", b"II", raw_aux=b"NMI\x01\x02"), rec(b"a", 0, b"AC", b"II", raw_aux=b"NM?\x01"),
                rec(b"a", 0, b"AC", b"II", raw_aux=b"XBBs" + struct.pack("<I", 9) + b"\0\0")):
        with pytest.raises(bam_reads.BadRecord):
            bam_reads.reads(rec(b"ok", 0, b"AC", b"II") + bad, b"RG")


def test_record_chain():
    a, b = rec(b"a", 0, b"ACGTA", b"IIIII"), rec(b"b", 0, b"AC", b"II")
    assert bam_reads.record_offsets(a + b) == [0, len(a)]

    def bad(buf, ordinal, offset):
        with pytest.raises(bam_reads.BadRecord) as e:
            bam_reads.reads(buf)
        assert (e.value.ordinal, e.value.offset) == (ordinal, offset)

    bad(a + b[:-1], 1, len(a))                                            # truncated last record
    bad(a + struct.pack("<I", len(b) - 3) + b[4:], 1, len(a))             # block_size one more than the buffer holds
    bad(a + struct.pack("<I", 31) + b[4:], 1, len(a))
    bad(a + b + b"\x01", 2, len(a) + len(b))
    bad(a + b[:12] + b"\0" + b[13:], 1, len(a))                           # l_read_name 0
    bad(a + b[:20] + struct.pack("<i", (1 << 31) - 1) + b[24:], 1, len(a))
    bad(a + b[:20] + struct.pack("<i", -1) + b[24:], 1, len(a))
    bad(a + b[:37] + b"x" + b[38:], 1, len(a))                            # the name's NUL
    bad(b[:37] + b"x" + b[38:] + a[:-1], 0, 0)                            # the earliest one is named


def test_to_fastq_is_consistent_with_the_records():
    rng = np.random.default_rng(5)
    flags = [0, 0x10, 0x100, 0x10, 0, 0x800, 0x10]
    rs = [(b"q%d" % k, f, rand_seq(rng, 30 + 7 * k), rand_qual(rng, 30 + 7 * k)) for k, f in enumerate(flags)]
    recs = b"".join(rec(n, f, s, q, [b"RG:Z:g%d" % (len(n))]) for n, f, s, q in rs)
    lines = bam_reads.to_fastq(recs, b"RG").split(b"\n")
    assert lines[-1] == b"" and len(lines) == 4 * 5 + 1
    kept = [r for r in rs if not r[1] & 0x900]
    for k, (n, f, s, q) in enumerate(kept):
        head, seq, plus, qual = lines[4 * k:4 * k + 4]
        _, codes, wq, _ = read_of(n, f, s, q)
        assert head == b"@" + n + b" RG:Z:g2" and plus == b"+" and qual == wq
        assert seq == bytes(b"ACGTN"[c] for c in codes)
