"""bwams/bam.py, the yardstick of the device BAM encoder (csrc/bam.hip), against hand-built bytes: reg2bin at the bin edges, htslib's
integer type choice, the record layout of the fields bwa prints (SEQ / QUAL '*', '=' RNEXT, negative TLEN, hard clips, unmapped reads at
their mate's position, pa:f), the header block, decode(encode(x)) == x, and the refusals."""
import struct

import numpy as np
import pytest

from bwams import bam

NAMES = [b"chr1", b"chr2", b"chrUn_alt"]


def test_reg2bin_edges():
    assert bam.reg2bin(-1, 0) == 4680                      # pos -1, end pos + 1: bam_endpos of an unplaced record
    assert bam.reg2bin(0, 1) == 4681 and bam.reg2bin(16383, 16384) == 4681
    assert bam.reg2bin(16384, 16385) == 4682
    assert bam.reg2bin(16383, 16385) == 585                 # spans a 16 kb edge: the 128 kb level
    assert bam.reg2bin(131071, 131073) == 73                # spans a 128 kb edge: the 1 Mb level
    assert bam.reg2bin(131072, 131073 + 16384) == 585 + 1
    assert bam.reg2bin(1048575, 1048577) == 9               # spans a 1 Mb edge: the 8 Mb level
    assert bam.reg2bin(1 << 20, (1 << 20) + 1) == 4681 + 64
    assert bam.reg2bin(0, 1 << 26) == 1 and bam.reg2bin(0, (1 << 26) + 1) == 0


@pytest.mark.parametrize("x,ty,raw", [(-129, b"s", struct.pack("<h", -129)), (-128, b"c", b"\x80"), (-32769, b"i", struct.pack("<i", -32769)),
                                      (0, b"C", b"\0"), (255, b"C", b"\xff"), (256, b"S", struct.pack("<H", 256)),
                                      (65535, b"S", b"\xff\xff"), (65536, b"I", struct.pack("<I", 65536)),
                                      (1 << 31, b"I", struct.pack("<I", 1 << 31))])
def test_int_type(x, ty, raw):
    assert bam.int_type(x) == (ty, raw)
    rec = bam.encode_records(b"r\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\tXY:i:%d\n" % x, NAMES)
    assert rec.endswith(b"XY" + ty + raw)


def _rec(refid, pos, name, mapq, bin_, cig, flag, seq_codes, l_seq, nref, pnext, tlen, qual, aux=b""):
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(name) + 1, mapq, bin_, len(cig), flag, l_seq, nref, pnext, tlen)
    body += name + b"\0" + b"".join(struct.pack("<I", c) for c in cig) + bytes(seq_codes) + qual + aux
    return struct.pack("<I", len(body)) + body


def test_record_layout_by_hand():
    # mapped, hard clip, '=' RNEXT, negative TLEN, pa:f, Z and A fields
    line = b"q1\t2145\tchr2\t100\t37\t3H4M1D2M\t=\t50\t-60\tACGTNA\t!#I+5?\tNM:i:1\tpa:f:0.955\tSA:Z:chr1,5,+,6M,0,0;\tXT:A:U\n"
    pos = 99
    end = pos + 4 + 1 + 2
    want = _rec(1, pos, b"q1", 37, bam.reg2bin(pos, end), [3 << 4 | 5, 4 << 4 | 0, 1 << 4 | 2, 2 << 4 | 0], 2145,
                [1 << 4 | 2, 4 << 4 | 8, 15 << 4 | 1], 6, 1, 49, -60, bytes([0, 2, 40, 10, 20, 30]),
                b"NMC\x01" + b"paf" + struct.pack("<f", np.float32(0.955)) + b"SAZchr1,5,+,6M,0,0;\0" + b"XTAU")
    assert bam.encode_records(line, NAMES) == want
    assert struct.unpack("<f", struct.pack("<f", np.float32(0.955)))[0] == np.float32(955 / 1000.0)
    # a secondary: SEQ and QUAL '*'; an unmapped mate at its mate's position; QUAL '*' with SEQ present
    sec = b"q2\t256\tchr1\t7\t0\t5M\t*\t0\t0\t*\t*\tAS:i:5\n"
    assert bam.encode_records(sec, NAMES) == _rec(0, 6, b"q2", 0, bam.reg2bin(6, 11), [5 << 4], 256, [], 0, -1, -1, 0, b"", b"ASC\x05")
    unm = b"q3\t133\tchr1\t1000\t0\t*\t=\t1000\t0\tACG\t*\n"
    assert bam.encode_records(unm, NAMES) == _rec(0, 999, b"q3", 0, bam.reg2bin(999, 1000), [], 133, [1 << 4 | 2, 4 << 4], 3, 0, 999, 0,
                                                   b"\xff\xff\xff")
    # fully unplaced: refID -1, pos -1, bin 4680
    un = bam.encode_records(b"q4\t4\t*\t0\t0\t*\t*\t0\t0\tAC\tII\n", NAMES)
    assert un == _rec(-1, -1, b"q4", 0, 4680, [], 4, [1 << 4 | 2], 2, -1, -1, 0, b"((")


def test_header_block():
    text = b"@SQ\tSN:chr1\tLN:10\n@PG\tID:bwa\n"
    blk = bam.header_block(text, [b"chr1", b"x"], [10, 3])
    want = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 2)
    want += struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 10) + struct.pack("<i", 2) + b"x\0" + struct.pack("<i", 3)
    assert blk == want
    h, refs, sam = bam.decode(blk)
    assert h == text and refs == [(b"chr1", 10), (b"x", 3)] and sam == b""


def _same_lines(a: bytes, b: bytes):
    """SAM texts equal, pa:f compared by float32 value"""
    la, lb = a.split(b"\n"), b.split(b"\n")
    assert len(la) == len(lb)
    for x, y in zip(la, lb):
        fx, fy = x.split(b"\t"), y.split(b"\t")
        assert len(fx) == len(fy)
        for u, v in zip(fx, fy):
            if u[2:5] == b":f:":
                assert u[:5] == v[:5] and np.float32(float(u[5:])) == np.float32(float(v[5:]))
            else:
                assert u == v


def test_round_trip():
    text = (b"q1\t2145\tchr2\t100\t37\t3H4M1D2M\t=\t50\t-60\tACGTNA\t!#I+5?\tNM:i:1\tpa:f:0.955\tXA:Z:chr1,+5,6M,0;\n"
            b"q1\t65\tchrUn_alt\t3\t60\t2S4M\tchr1\t9\t0\tGGTTAC\tIIIIII\tXS:i:-40000\tXB:i:4294967295\tRG:Z:grp\n"
            b"q2\t256\tchr1\t7\t0\t5M\t*\t0\t0\t*\t*\tAS:i:5\n"
            b"q3\t133\tchr1\t1000\t0\t*\t=\t1000\t0\tACG\t*\n"
            b"q4\t4\t*\t0\t0\t*\t*\t0\t0\tRYKMSWBDHV=\tABCDEFGHIJK\tXR:Z:an anno\tpa:f:1.000\n"
            b"empty\t4\t*\t0\t0\t*\t*\t0\t0\t\t*\n")
    enc = bam.encode_records(text, NAMES)
    assert len(bam.split_records(enc)) == 6
    _, _, back = bam.decode(enc, NAMES)
    _same_lines(back, text.replace(b"\t\t*\n", b"\t*\t*\n"))          # an empty SEQ reads back as '*', as samtools prints it
    hdr = bam.header_block(b"@HD\n", NAMES, [5, 6, 7])
    h, refs, back2 = bam.decode(hdr + enc)
    assert h == b"@HD\n" and [r for r, _ in refs] == NAMES and back2 == back


@pytest.mark.parametrize("line", [
    b"r\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\t1:N:0:ACGT\n",                # an Illumina comment copied as is
    b"r\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\tBC:B:c,1,2\n",                # B arrays
    b"r\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\tXX:i:4294967296\n",           # beyond uint32
    b"r\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\tXX:i:-2147483649\n",          # beyond int32
    b"r\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\tXX:A:ab\n",
    b"r\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\tXX:f:1e5\n",
    b"r\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\t\n",                           # an empty field after a tab
    b"r\t4\t*\t0\t0\t*\t*\t0\t0\tAC\tI\n",                            # SEQ / QUAL lengths differ
    b"r\t4\tchrX\t1\t0\t*\t*\t0\t0\tA\tI\n",                          # not a sequence of the index
    b"r\t4\t*\t0\t0\t*\t*\t0\tA\tI\n",                                # ten fields
    b"x" * 255 + b"\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n",                 # a 255-byte name
])
def test_refusals(line):
    ok = b"ok\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n"
    with pytest.raises(bam.BamRefusal) as e:
        bam.encode_records(ok + ok + line + ok, NAMES)
    assert e.value.line == 2


def test_limits_that_pass():
    assert bam.encode_records(b"x" * 254 + b"\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\tXX:i:-2147483648\tXY:i:4294967295\n", NAMES)
    assert bam.encode_records(b"r\t0\tchr1\t1\t0\t65535M\t*\t0\t0\t*\t*\n", NAMES)
