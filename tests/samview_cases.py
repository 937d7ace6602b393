"""Builders shared by test_samview.py and test_gpu_samview.py: a record builder that can make what no encoder makes (rule V6's
faults, B arrays, every limit), the hand-written (record, line) pairs of rules V3-V5 and V7 with the lines as literal bytes, one
record per refusal reason, the named floats of rule V5, and canonical SAM texts for the round trip through bwams.bam's encoder."""
import struct

import numpy as np

import bam_query_cases as Q
from test_bam import NAMES, _rec                      # chr1, chr2, chrUn_alt; the record laid out field by field

_CODE = {c: i for i, c in enumerate(b"=ACMGRSVTWYHKDBN")}


def f32(x) -> bytes:
    return struct.pack("<f", np.float32(x))


def rec(name=b"r", flag=0, refid=-1, pos=-1, mapq=0, cigar=(), seq=b"", qual=None, nrefid=-1, pnext=-1, tlen=0, aux=b"",
        l_name=None, l_seq=None, name_raw=None, tail=None) -> bytes:
    """One record, block_size included.  cigar: (length, op code) pairs; seq: bases as text; qual: phred bytes, None
    for 0xFF; name_raw: the name's bytes as they lie (no NUL added); l_name / l_seq: the counts written, whatever the bytes;
    tail: everything behind the CIGAR instead of SEQ, QUAL and aux."""
    nm = name_raw if name_raw is not None else name + b"\0"
    ops = [n << 4 | o for n, o in cigar]
    codes = [_CODE[c] for c in seq] + [0]
    packed = bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(seq), 2))
    q = b"\xff" * len(seq) if qual is None else bytes(qual)
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(nm) if l_name is None else l_name, mapq, 4680, len(ops), flag,
                       len(seq) if l_seq is None else l_seq, nrefid, pnext, tlen)
    body += nm + b"".join(struct.pack("<I", c) for c in ops) + (packed + q + aux if tail is None else tail)
    return struct.pack("<I", len(body)) + body


# ---- rules V3-V5, V7: (what it covers, record, expected line), the lines written by hand ----
_Q16 = bytes(range(16))
LITERALS = [
    ("unmapped, * everywhere",
     _rec(-1, -1, b"u", 0, 4680, [], 4, [], 0, -1, -1, 0, b""),
     b"u\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"),
    ("RNEXT =, hard clip, negative TLEN, even l_seq",
     _rec(1, 99, b"q1", 37, 0, [3 << 4 | 5, 4 << 4 | 0, 1 << 4 | 2, 2 << 4 | 0], 2145, [0x12, 0x48, 0xF1], 6, 1, 49, -60,
          bytes([0, 2, 40, 10, 20, 30])),
     b"q1\t2145\tchr2\t100\t37\t3H4M1D2M\t=\t50\t-60\tACGTNA\t!#I+5?\n"),
    ("RNEXT another reference",
     _rec(2, 2, b"q1", 60, 0, [2 << 4 | 4, 4 << 4 | 0], 65, [0x44, 0x88, 0x12], 6, 0, 8, 0, bytes([40] * 6)),
     b"q1\t65\tchrUn_alt\t3\t60\t2S4M\tchr1\t9\t0\tGGTTAC\tIIIIII\n"),
    ("RNEXT * on a mapped record, SEQ and QUAL *",
     _rec(0, 6, b"q2", 0, 0, [5 << 4], 256, [], 0, -1, -1, 0, b"", b"ASC\x05"),
     b"q2\t256\tchr1\t7\t0\t5M\t*\t0\t0\t*\t*\tAS:i:5\n"),
    ("QUAL 0xFF, odd l_seq",
     _rec(0, 999, b"q3", 0, 0, [], 133, [0x12, 0x40], 3, 0, 999, 0, b"\xff\xff\xff"),
     b"q3\t133\tchr1\t1000\t0\t*\t=\t1000\t0\tACG\t*\n"),
    ("every CIGAR op, MAPQ 255",
     _rec(0, 0, b"c", 255, 0, [(k + 1) << 4 | k for k in range(9)], 0, [0x10], 1, -1, -1, 0, b"\0"),
     b"c\t0\tchr1\t1\t255\t1M2I3D4N5S6H7P8=9X\t*\t0\t0\tA\t!\n"),
    ("every SEQ code",
     _rec(-1, -1, b"s", 0, 4680, [], 4, [0x01, 0x23, 0x45, 0x67, 0x89, 0xAB, 0xCD, 0xEF], 16, -1, -1, 0, _Q16),
     b"s\t4\t*\t0\t0\t*\t*\t0\t0\t=ACMGRSVTWYHKDBN\t!\"#$%&'()*+,-./0\n"),
    ("every aux type",
     _rec(-1, -1, b"a", 0, 4680, [], 4, [], 0, -1, -1, 0, b"",
          b"XAAq" + b"Xcc\x80" + b"XCC\xff" + b"Xss" + struct.pack("<h", -32768) + b"XSS" + struct.pack("<H", 65535) +
          b"Xii" + struct.pack("<i", -(1 << 31)) + b"XII" + struct.pack("<I", (1 << 32) - 1) + b"XZZa b\0" + b"XHH1AE3\0" +
          b"Xff" + f32(0.955)),
     b"a\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\tXA:A:q\tXc:i:-128\tXC:i:255\tXs:i:-32768\tXS:i:65535\tXi:i:-2147483648\tXI:i:4294967295"
     b"\tXZ:Z:a b\tXH:H:1AE3\tXf:f:0.955\n"),
    ("a B array of each subtype",
     _rec(-1, -1, b"b", 0, 4680, [], 4, [], 0, -1, -1, 0, b"",
          b"B1Bc" + struct.pack("<Ibb", 2, -1, 2) + b"B2BC" + struct.pack("<IBB", 2, 0, 255) + b"B3Bs" + struct.pack("<Ih", 1, -300) +
          b"B4BS" + struct.pack("<IHH", 2, 65535, 1) + b"B5Bi" + struct.pack("<Ii", 1, -70000) +
          b"B6BI" + struct.pack("<II", 1, 4000000000) + b"B7Bf" + struct.pack("<I", 3) + f32(1.5) + f32(-0.25) + f32(1e10)),
     b"b\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\tB1:B:c,-1,2\tB2:B:C,0,255\tB3:B:s,-300\tB4:B:S,65535,1\tB5:B:i,-70000\tB6:B:I,4000000000"
     b"\tB7:B:f,1.5,-0.25,1e+10\n"),
    ("a B count of 0, a field behind it",
     _rec(-1, -1, b"z", 0, 4680, [], 4, [], 0, -1, -1, 0, b"", b"B0Bc\0\0\0\0" + b"NMC\x01"),
     b"z\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\tB0:B:c\tNM:i:1\n"),
    ("nothing is interpreted: a tab in the name, a newline in a Z value, CG printed as a tag, an empty Z",
     _rec(0, 0, b"a\tb", 1, 0, [4 << 4 | 4, 100 << 4 | 3], 0, [0x12, 0x48], 4, -1, -1, 0, bytes([1, 2, 3, 4]),
          b"XZZx\ny\0" + b"CGBI" + struct.pack("<II", 1, 16) + b"XEZ\0"),
     b"a\tb\t0\tchr1\t1\t1\t4S100N\t*\t0\t0\tACGT\t\"#$%\tXZ:Z:x\ny\tCG:B:I,16\tXE:Z:\n"),
    ("floats: special values, both forms, the ties",
     _rec(-1, -1, b"f", 0, 4680, [], 4, [], 0, -1, -1, 0, b"",
          b"f1f" + f32(np.inf) + b"f2f" + f32(-np.inf) + b"f3f" + struct.pack("<I", 0x7FC00000) + b"f4f" + f32(1e-5) +
          b"f5f" + f32(100000) + b"f6f" + f32(1e6) + b"f7f" + f32(1234565) + b"f8f" + f32(1234575) + b"f9f" + f32(-0.0) +
          b"fAf" + f32(0.0001) + b"fBf" + f32(999999.5) + b"fCf" + struct.pack("<I", 0xFFC00000)),
     b"f\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\tf1:f:inf\tf2:f:-inf\tf3:f:nan\tf4:f:1e-05\tf5:f:100000\tf6:f:1e+06\tf7:f:1.23456e+06"
     b"\tf8:f:1.23458e+06\tf9:f:-0\tfA:f:0.0001\tfB:f:1e+06\tfC:f:-nan\n"),
]

# ---- rule V5: the floats by name, as float32 values or bit patterns ----
FLT_MIN, FLT_MAX = np.float32(1.17549435e-38), np.float32(3.40282347e38)
NAMED_FLOATS = [np.float32(x) for x in (1234565, 1234575, 9999995, 999999.5, 99999.95, 100000, 999999, 1e6, 0.0001,
                                        np.nextafter(np.float32(0.0001), np.float32(0)), 1e-5, FLT_MIN, FLT_MAX, 0.0, -0.0,
                                        np.inf, -np.inf, np.nan, 0.955, 1.5, 16777216, 0.1)]
NAMED_BITS = [1, 0x80000001, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x007FFFFF]           # the smallest subnormal, NaNs, the largest subnormal


def float_bits() -> np.ndarray:
    """Every exponent byte, times the mantissas 0, 1, 0x400000, 0x7FFFFF and 64 seeded random ones, times both signs, then the
    named ones: uint32 bit patterns."""
    rng = np.random.default_rng(5)
    man = np.concatenate([np.array([0, 1, 0x400000, 0x7FFFFF], np.uint32), rng.integers(0, 1 << 23, 64).astype(np.uint32)])
    e = np.arange(256, dtype=np.uint32)[:, None] << 23
    pos = (e | man[None, :]).reshape(-1)
    named = np.concatenate([np.array(NAMED_FLOATS, np.float32).view(np.uint32), np.array(NAMED_BITS, np.uint32)])
    return np.concatenate([pos, pos | np.uint32(0x80000000), named]).astype(np.uint32)


# ---- rule V6: (what, record, reason); every record passes the front door's chain check (block_size, refID >= -1, name and CIGAR inside) ----
OK = rec(b"ok", 4, seq=b"ACGT", qual=[30] * 4, aux=b"NMC\x00")
N_REF = len(NAMES)
REFUSALS = [
    ("refID == n_ref", rec(refid=N_REF, pos=0), 1),
    ("next refID < -1", rec(refid=0, pos=0, nrefid=-2), 1),
    ("next refID == n_ref", rec(nrefid=N_REF), 1),
    ("l_read_name == 0", rec(name_raw=b"", seq=b"AC", qual=[1, 2]), 2),
    ("the name's last byte is not NUL", rec(name_raw=b"ab"), 2),
    ("a NUL inside the name", rec(name_raw=b"a\0b\0"), 2),
    ("a long name without its NUL", rec(name_raw=b"x" * 40), 2),
    ("CIGAR op code 9", rec(refid=0, pos=0, cigar=[(5, 0), (1, 9)]), 3),
    ("op code 15 in the second group step", rec(refid=0, pos=0, cigar=[(5, 0)] * 20 + [(1, 15)]), 3),
    ("l_seq < 0", rec(l_seq=-1), 4),
    ("SEQ and QUAL pass the record's end", rec(l_seq=100, tail=b"\x11" * 20), 4),
    ("QUAL one byte short", rec(l_seq=4, tail=b"\x12\x48" + b"\x05" * 3), 4),
    ("aux type d", rec(aux=b"XDd" + struct.pack("<d", 1.0)), 5),
    ("a Z value without its NUL", rec(aux=b"XZZabcdefghijklmnopqrstuvwxyz"), 5),
    ("an H value without its NUL", rec(aux=b"NMC\x01XHH1A"), 5),
    ("a B subtype that is none of cCsSiIf", rec(aux=b"XBBA" + struct.pack("<I", 1) + b"x"), 5),
    ("a B count past the record's end", rec(aux=b"XBBs" + struct.pack("<I", 3) + b"\0" * 4), 5),
    ("a B header cut off", rec(aux=b"XBBc\0\0"), 5),
    ("an i value cut off", rec(aux=b"NMi\x01\x02"), 5),
    ("two stray bytes behind the last field", rec(aux=b"NMC\x01XY"), 5),
    ("an unknown type", rec(aux=b"XQq\x01"), 5),
]


# ---- canonical SAM texts: what view(encode_records(text)) must give back byte for byte ----
def canonical_texts():
    """(names, text) pairs: test_bam.py's round-trip lines in the form a view prints (%g floats, * for an empty SEQ), and the
    lines bam_query_cases.py builds."""
    t1 = (b"q1\t2145\tchr2\t100\t37\t3H4M1D2M\t=\t50\t-60\tACGTNA\t!#I+5?\tNM:i:1\tpa:f:0.955\tXA:Z:chr1,+5,6M,0;\n"
          b"q1\t65\tchrUn_alt\t3\t60\t2S4M\tchr1\t9\t0\tGGTTAC\tIIIIII\tXS:i:-40000\tXB:i:4294967295\tRG:Z:grp\n"
          b"q2\t256\tchr1\t7\t0\t5M\t*\t0\t0\t*\t*\tAS:i:5\n"
          b"q3\t133\tchr1\t1000\t0\t*\t=\t1000\t0\tACG\t*\n"
          b"q4\t4\t*\t0\t0\t*\t*\t0\t0\tRYKMSWBDHV=\tABCDEFGHIJK\tXR:Z:an anno\tpa:f:1\tXT:A:U\tXH:H:00FF\tXE:Z:\n"
          b"empty\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"
          + b"x" * 254 + b"\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\tXX:i:-2147483648\tXY:i:4294967295\tXc:i:-128\tXs:i:-129\tXC:i:255\tXS:i:256\n"
          b"r\t0\tchr1\t1\t0\t65535M\t*\t0\t0\t*\t*\n"
          b"f\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\tf1:f:0.5\tf2:f:123456\tf3:f:-0.0625\tf4:f:0.001\tf5:f:100000\n")
    rng = np.random.default_rng(23)
    t2 = b"".join(ln + b"\n" for ln in Q.named_lines(rng) + Q.background(rng, 120, unplaced=3))
    return [(NAMES, t1), (Q.NAMES, t2)]
