"""The depth rules (include/bwams.h above bwams_depth_open) on hand-built records: bwams/depth.py against depths, query results and
texts written out here.  tests/test_gpu_depth.py runs the same records through the C-ABI."""
import struct

import numpy as np
import pytest

from bwams import bam, depth

OPS = {c: i for i, c in enumerate("MIDNSHP=X")}


def rec(refid: int, pos: int, cigar, flag: int = 0, mapq: int = 60, name: bytes = b"r", qual: int | None = None, pad: int = 0) -> bytes:
    """One BAM record.  cigar: text ("3M2D3M"; "" for none) or a list of (length, op code), which may hold codes SAM text cannot.
    qual: every base's quality, with a sequence of the CIGAR's query length (None: no sequence).  pad: bytes of a trailing Z field."""
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
    l_seq = sum(n for n, op in ops if op in (0, 1, 4, 7, 8)) if qual is not None else 0
    rlen = sum(n for n, op in ops if op in (0, 2, 3, 7, 8))
    end = pos + rlen if rlen and not flag & 4 else pos + 1
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(name) + 1, mapq, bam.reg2bin(max(pos, 0), max(end, 1)) & 0xFFFF, len(ops), flag, l_seq,
                       -1, -1, 0)
    body += name + b"\0" + b"".join(struct.pack("<I", n << 4 | op) for n, op in ops)
    body += b"\x11" * ((l_seq + 1) // 2) + bytes([qual or 0]) * l_seq
    if pad:
        body += b"XZZ" + b"p" * (pad - 4) + b"\0"
    return struct.pack("<I", len(body)) + body


L_REF = [20, 1, 0, 12]
NAMES = [b"c0", b"c1", b"c2", b"c3"]
HAND = [
    rec(0, 2, "5M"),                          # [2, 7)
    rec(0, 0, "2S3M1I2M"),                    # M I M touch on the reference: [0, 5)
    rec(0, 4, "3M2D3M"),                      # [4, 7) [9, 12); with deletions [4, 12)
    rec(0, 10, "2M3N2M"),                     # N parts them: [10, 12) [15, 17)
    rec(0, 18, "5M"),                         # runs off the end: [18, 20)
    rec(0, 25, "3M"),                         # POS beyond the end: counts, covers nothing
    rec(0, 15, "2H1=1X2P1M3S"),               # [15, 18)
    rec(0, 0, "10M", flag=0x400),             # a duplicate: excluded
    rec(0, 6, "2M", flag=0x800),              # supplementary: counts, [6, 8)
    rec(1, 0, "4M"),                          # a reference of one base
    rec(2, 0, "3M"),                          # a reference of no base: counts, covers nothing
    rec(3, 11, "1M"),                         # the last base
    rec(3, 0, "1M"),                          # the first base, next to reference 1's and 2's ends in memory
    rec(-1, 0, "5M"), rec(4, 0, "5M"), rec(0, 3, ""),      # skipped: no reference, refID == n_ref, no CIGAR
]
N_COUNTED = 12
WANT = [[1, 1, 2, 2, 3, 2, 3, 1, 0, 1, 2, 2, 0, 0, 0, 2, 2, 1, 1, 1], [1], [], [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]]
WANT_DEL = [[1, 1, 2, 2, 3, 2, 3, 2, 1, 1, 2, 2, 0, 0, 0, 2, 2, 1, 1, 1]] + WANT[1:]
SUMMARY = [dict(length=20, bases=27, min=0, max=3), dict(length=1, bases=1, min=1, max=1), dict(length=0, bases=0, min=0, max=0),
           dict(length=12, bases=2, min=0, max=1)]
TEXT_SUMMARY = ("chrom\tlength\tbases\tmean\tmin\tmax\n" "c0\t20\t27\t1.35\t0\t3\n" "c1\t1\t1\t1.00\t1\t1\n" "c2\t0\t0\t0.00\t0\t0\n"
                "c3\t12\t2\t0.17\t0\t1\n" "total\t33\t30\t0.91\t0\t3\n")
TEXT_DIST = ("total\t3\t0.0606\n" "total\t2\t0.2727\n" "total\t1\t0.5758\n" "total\t0\t1.0000\n"
             "c0\t3\t0.1000\n" "c0\t2\t0.4500\n" "c0\t1\t0.8000\n" "c0\t0\t1.0000\n"
             "c1\t1\t1.0000\n" "c1\t0\t1.0000\n"
             "c3\t1\t0.1667\n" "c3\t0\t1.0000\n")
TEXT_WINDOWS_8 = ("c0\t0\t8\t1.88\n" "c0\t8\t16\t0.88\n" "c0\t16\t20\t1.25\n" "c1\t0\t1\t1.00\n" "c3\t0\t8\t0.12\n" "c3\t8\t12\t0.25\n")

# the example of include/bwams.h's rule 11: c1 with depths 2 2 2 2 2 0 0 0 0 1, c2 of length 0
EX_L_REF, EX_NAMES = [10, 0], [b"c1", b"c2"]
EX_RECS = [rec(0, 0, "5M"), rec(0, 0, "5M"), rec(0, 9, "1M")]
EX_SUMMARY = "chrom\tlength\tbases\tmean\tmin\tmax\n" "c1\t10\t11\t1.10\t0\t2\n" "c2\t0\t0\t0.00\t0\t0\n" "total\t10\t11\t1.10\t0\t2\n"
EX_DIST = "total\t2\t0.5000\n" "total\t1\t0.6000\n" "total\t0\t1.0000\n" "c1\t2\t0.5000\n" "c1\t1\t0.6000\n" "c1\t0\t1.0000\n"
EX_WINDOWS_4 = "c1\t0\t4\t2.00\n" "c1\t4\t8\t0.50\n" "c1\t8\t10\t0.50\n"


def hand(**kw) -> depth.Depth:
    d = depth.Depth(L_REF, **kw)
    assert d.add(b"".join(HAND)) == N_COUNTED
    return d.finish()


def test_hand_depths():
    assert [x.tolist() for x in hand().depth] == WANT
    assert [x.tolist() for x in hand(count_deletions=True).depth] == WANT_DEL
    assert hand().summary() == SUMMARY


def test_filters():
    d = depth.Depth(L_REF, exclude=0x704 | 0x800)
    assert d.add(b"".join(HAND)) == N_COUNTED - 1
    assert d.finish().depth[0].tolist()[6:8] == [2, 0]
    d = depth.Depth([10], min_mapq=30)
    assert d.add(rec(0, 0, "3M", mapq=29) + rec(0, 1, "3M", mapq=30)) == 1
    assert d.finish().depth[0].tolist() == [0, 1, 1, 1, 0, 0, 0, 0, 0, 0]
    for bit in (0x4, 0x100, 0x200, 0x400):
        d = depth.Depth([10])
        assert d.add(rec(0, 0, "3M", flag=bit) + rec(0, 0, "1M", flag=0x1 | 0x10 | 0x800)) == 1
        assert d.finish().depth[0].tolist()[:3] == [1, 0, 0]


def test_bad_op_refuses_the_call():
    d = depth.Depth([10])
    d.add(rec(0, 0, "3M"))
    with pytest.raises(depth.DepthRefusal) as e:
        d.add(rec(0, 0, "2M") + rec(0, 0, "2M") + rec(-1, 0, [(2, 0), (1, 9)], flag=0x4) + rec(0, 0, [(1, 12)]))
    assert e.value.record == 2                                                 # counted or not; nothing of the call is added
    assert d.finish().depth[0].tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0, 0]


def test_queries():
    d = hand()
    assert d.hist(-1, 4).tolist() == [14, 10, 7, 2] and d.hist(-1, 3).tolist() == [14, 10, 9] and d.hist(-1, 2).tolist() == [14, 19]
    assert d.hist(0, 8).tolist() == [4, 7, 7, 2, 0, 0, 0, 0] and d.hist(2, 2).tolist() == [0, 0] and d.hist(1, 2).tolist() == [0, 1]
    assert d.windows(8).tolist() == [15, 7, 5, 1, 1, 1]
    assert d.windows(1).tolist() == WANT[0] + WANT[1] + WANT[3]
    assert d.windows(100).tolist() == [27, 1, 2] and d.windows(20).tolist() == [27, 1, 2] and d.windows(12).tolist() == [20, 7, 1, 2]
    s, v = d.runs(0, 3, 12)
    assert s.tolist() == [3, 4, 5, 6, 7, 8, 9, 10] and v.tolist() == [2, 3, 2, 3, 1, 0, 1, 2]       # position 2 has depth 2 as well
    s, v = d.runs(3, 0, 12)
    assert s.tolist() == [0, 1, 11] and v.tolist() == [1, 0, 1]
    assert d.runs(0, 5, 5)[0].tolist() == []


def test_accumulation_and_reset():
    d = depth.Depth(L_REF)
    for part in (HAND[:5], HAND[5:11], HAND[11:]):
        d.add(b"".join(part))
    assert [x.tolist() for x in d.finish().depth] == WANT
    d.reset()
    d.add(b"".join(reversed(HAND)))
    assert [x.tolist() for x in d.finish().depth] == WANT


def test_texts():
    d = hand()
    assert d.text(NAMES, depth.TEXT_SUMMARY) == TEXT_SUMMARY
    assert d.text(NAMES, depth.TEXT_DIST) == TEXT_DIST and d.text(NAMES, depth.TEXT_DIST, 4) == TEXT_DIST
    assert d.text(NAMES, depth.TEXT_WINDOWS, 8) == TEXT_WINDOWS_8
    e = depth.Depth(EX_L_REF)
    e.add(b"".join(EX_RECS))
    e.finish()
    assert e.depth[0].tolist() == [2, 2, 2, 2, 2, 0, 0, 0, 0, 1]
    assert e.text(EX_NAMES, depth.TEXT_SUMMARY) == EX_SUMMARY and e.text(EX_NAMES, depth.TEXT_DIST) == EX_DIST
    assert e.text(EX_NAMES, depth.TEXT_WINDOWS, 4) == EX_WINDOWS_4
    assert e.text(EX_NAMES, depth.TEXT_DIST, 2) == "total\t1\t0.6000\ntotal\t0\t1.0000\nc1\t1\t0.6000\nc1\t0\t1.0000\n"   # the last bin is open-ended
    z = depth.Depth([]).finish()
    assert z.text([], depth.TEXT_SUMMARY) == "chrom\tlength\tbases\tmean\tmin\tmax\ntotal\t0\t0\t0.00\t0\t0\n"
    assert z.text([], depth.TEXT_DIST) == "" and z.text([], depth.TEXT_WINDOWS, 5) == ""


def test_rec_matches_the_sam_encoder():
    line = b"\t".join([b"r", b"16", b"c0", b"5", b"37", b"2S3M1I2M", b"*", b"0", b"0", b"*", b"*"])
    assert rec(0, 4, "2S3M1I2M", flag=16, mapq=37) == bam.encode_record(line, {b"c0": 0})
    assert np.array_equal(depth.fields(rec(3, 7, "4M2D", flag=99, mapq=5))[:4], (3, 7, 5, 99))
