"""bwams/qc.py, the numpy restatement of the alignment-QC rules (include/bwams.h above bwams_qc_open), against the hand-checked
example of the header, built as real BAM bytes; every refusal of rule 1 with its record and reason; NM in every form rule 5 names.
tests/test_gpu_qc.py and tests/test_qc_text_host.py take their records and expectations from here."""
import struct

import numpy as np
import pytest

from bwams import bam, qc

OPS = {c: k for k, c in enumerate("MIDNSHP=X")}
CODE = {c: k for k, c in enumerate("=ACMGRSVTWYHKDBN")}


def aux_int(tag: bytes, t: bytes, v: int) -> bytes:
    return tag + t + struct.pack({b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}[t], v)


def qrec(flag, refid, pos, mapq, nref, npos, tlen, cigar, seq, qual=None, nm=None, aux: bytes = b"", name: bytes = b"r") -> bytes:
    """One BAM record.  cigar: text ("3M2D3M"; "" for none) or a list of (length, op code); seq: letters, or 4-bit codes; qual: a list
    (None: 0xFF bytes); nm: an NM:C field in front of `aux`, the aux area's other bytes as they are."""
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
    codes = [CODE[c] for c in seq] if isinstance(seq, str) else [int(c) for c in seq]
    l_seq = len(codes)
    codes = codes + [0] * (l_seq & 1)
    qual = [0xFF] * l_seq if qual is None else list(qual)
    assert len(qual) == l_seq
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(name) + 1, mapq, 4680, len(ops), flag, l_seq, nref, npos, tlen)
    body += name + b"\0" + b"".join(struct.pack("<I", n << 4 | op) for n, op in ops)
    body += bytes(codes[k] << 4 | codes[k + 1] for k in range(0, len(codes), 2)) + bytes(qual)
    body += (aux_int(b"NM", b"C", nm) if nm is not None else b"") + aux
    return struct.pack("<I", len(body)) + body


# the header's example: (FLAG, refID, POS, MAPQ, next_refID, next_pos, TLEN, CIGAR, SEQ, QUAL, NM)
HAND_OPT = dict(exclude=0x900, max_cycle=64, max_isize=100)
HAND = [qrec(99, 0, 10, 60, 0, 110, 104, "4M", "ACGT", [30, 30, 20, 10], 0),
        qrec(147, 0, 110, 60, 0, 10, -104, "2M1I2M", "ACGTA", [40, 40, 30, 20, 10], 1),
        qrec(73, 0, 50, 30, 0, 50, 0, "1S3M", "NACG", [2, 30, 30, 30], 1),
        qrec(133, 0, 50, 0, 0, 50, 0, "", "TTT", [10, 10, 10]),
        qrec(2064, 0, 200, 5, -1, -1, 0, "2M2D1M2H", "ACG", [30, 30, 30], 2),
        qrec(1536, 0, 5, 0, -1, -1, 0, "3M", "GGG", None, 0),
        qrec(81, 0, 300, 60, 0, 340, 42, "2M", "CC", [30, 70]),
        qrec(97, 0, 400, 4, 1, 7, 0, "2M", "AT", [30, 30], 0),
        qrec(161, 1, 7, 9, 0, 400, 0, "2M", "GG", [30, 30], 0),
        qrec(65, 0, 500, 60, 0, 520, 22, "2M", "AA", [30, 30], 0)]
HAND_FLAGS = [[9, 8, 0, 1, 0, 0, 8, 7, 8, 5, 3, 2, 6, 1, 2, 1], [1, 1, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]]
HAND_SCALARS = dict(reads=9, bases=27, mapped=8, bases_mapped=23, clipped=1, nm_sum=2, nm_missing=1, qual_sum=632, qual_bases=24,
                    bases_over=0, no_qual=1)
HAND_FLAGSTAT = ("9 + 1 in total (QC-passed reads + QC-failed reads)\n" "8 + 1 primary\n" "0 + 0 secondary\n" "1 + 0 supplementary\n"
                 "0 + 1 duplicates\n" "0 + 1 primary duplicates\n" "8 + 1 mapped (88.89% : 100.00%)\n"
                 "7 + 1 primary mapped (87.50% : 100.00%)\n" "8 + 0 paired in sequencing\n" "5 + 0 read1\n" "3 + 0 read2\n"
                 "2 + 0 properly paired (25.00% : N/A)\n" "6 + 0 with itself and mate mapped\n" "1 + 0 singletons (12.50% : N/A)\n"
                 "2 + 0 with mate mapped to a different chr\n" "1 + 0 with mate mapped to a different chr (mapQ>=5)\n")


def _q64(**bins) -> str:
    row = [0] * 64
    for k, v in bins.items():
        row[int(k[1:])] = v
    return "\t".join(str(v) for v in row)


HAND_STATS = ("SN\treads\t9\n" "SN\tbases\t27\n" "SN\tmapped\t8\n" "SN\tbases_mapped\t23\n" "SN\tclipped\t1\n" "SN\tnm_sum\t2\n"
              "SN\tnm_missing\t1\n" "SN\tqual_sum\t632\n" "SN\tqual_bases\t24\n" "SN\tbases_over\t0\n" "SN\tno_qual\t1\n"
              "SN\terror_rate\t8.695652e-02\n" "SN\taverage_quality\t26.3\n" "SN\tinsert_size_n\t2\n" "SN\tinsert_size_mean\t32.0\n"
              "SN\tinsert_size_sd\t10.0\n" "SN\tinsert_size_median\t22\n" "RL\t2\t3\t1\n" "RL\t3\t1\t1\n" "RL\t4\t2\t0\n" "RL\t5\t0\t1\n"
              "FFQ\t1\t" + _q64(b2=1, b30=3, b63=1) + "\n" "FFQ\t2\t" + _q64(b30=5) + "\n" "FFQ\t3\t" + _q64(b20=1, b30=1) + "\n"
              "FFQ\t4\t" + _q64(b10=1, b30=1) + "\n"
              "LFQ\t1\t" + _q64(b10=2, b30=1) + "\n" "LFQ\t2\t" + _q64(b10=1, b20=1, b30=1) + "\n" "LFQ\t3\t" + _q64(b10=1, b30=1) + "\n"
              "LFQ\t4\t" + _q64(b40=1) + "\n" "LFQ\t5\t" + _q64(b40=1) + "\n"
              "GCC\t1\t3\t0\t2\t0\t1\t0\t0\t1\t2\t0\n" "GCC\t2\t2\t1\t2\t1\t0\t1\t0\t1\t1\t0\n" "GCC\t3\t0\t1\t2\t0\t0\t0\t1\t0\t1\t0\n"
              "GCC\t4\t0\t0\t1\t1\t0\t0\t0\t1\t0\t0\n" "GCC\t5\t0\t0\t0\t0\t0\t0\t0\t0\t1\t0\n"
              "MAPQ\t0\t1\n" "MAPQ\t4\t1\n" "MAPQ\t9\t1\n" "MAPQ\t30\t1\n" "MAPQ\t60\t4\n"
              "IS\t22\t0\t0\t1\n" "IS\t42\t0\t1\t0\n" "IS\t100\t1\t0\t0\n" "ID\t1\t1\t0\n")
EMPTY_FLAGSTAT = "".join("0 + 0 %s%s\n" % (label, " (N/A : N/A)" if k in (6, 7, 11, 13) else "") for k, label in enumerate(qc.FLAGSTAT_LABELS))
EMPTY_STATS = "".join("SN\t%s\t0\n" % n for n in qc.SCALARS + ("error_rate", "average_quality", "insert_size_n", "insert_size_mean",
                                                               "insert_size_sd", "insert_size_median"))


def hand() -> qc.Qc:
    q = qc.Qc(**HAND_OPT)
    assert q.add(b"".join(HAND)) == 9
    return q


def test_hand_example():
    q = hand()
    flags, scalars = q.summary()
    assert flags.tolist() == HAND_FLAGS
    assert {n: int(scalars[k]) for k, n in enumerate(qc.SCALARS)} == HAND_SCALARS and not scalars[11:].any()
    qual = q.table(qc.QUAL).reshape(2, 64, 64)
    base = q.table(qc.BASE).reshape(2, 64, 5)
    assert qual[0, 0, 63] == 1 and qual[0, 0, 30] == 3 and qual[0, 0, 2] == 1 and qual[1, 0, 10] == 2 and qual[1, 4, 40] == 1
    assert base[0, 0].tolist() == [3, 0, 2, 0, 1] and base[1, 0, 3] == 2 and base[1, 0, 2] == 1
    assert int(qual.sum()) == 24 and int(base.sum()) == 27
    mapq = q.table(qc.MAPQ)
    assert {int(k): int(mapq[k]) for k in np.flatnonzero(mapq)} == {60: 4, 30: 1, 9: 1, 4: 1, 0: 1}
    rl = q.table(qc.RL).reshape(2, 65)
    assert [{int(k): int(r[k]) for k in np.flatnonzero(r)} for r in rl] == [{2: 3, 3: 1, 4: 2}, {2: 1, 3: 1, 5: 1}]
    indel = q.table(qc.INDEL).reshape(2, 65)
    assert indel[0, 1] == 1 and int(indel.sum()) == 1                            # the supplementary record's deletion is filtered out
    isize = q.table(qc.ISIZE).reshape(3, 101)
    assert isize[0, 100] == 1 and isize[1, 42] == 1 and isize[2, 22] == 1 and int(isize.sum()) == 3
    assert q.insert_size() == (2, 32.0, 10.0, 22)
    assert q.text(qc.TEXT_FLAGSTAT) == HAND_FLAGSTAT
    assert q.text(qc.TEXT_STATS) == HAND_STATS


def test_empty_reset_and_accumulation():
    q = qc.Qc()
    assert q.text(qc.TEXT_FLAGSTAT) == EMPTY_FLAGSTAT and q.text(qc.TEXT_STATS) == EMPTY_STATS
    one, parts = hand(), qc.Qc(**HAND_OPT)
    assert [parts.add(b"".join(HAND[a:b])) for a, b in ((0, 4), (4, 4), (4, 10))] == [4, 0, 5]
    assert parts.text(qc.TEXT_STATS) == HAND_STATS and all(np.array_equal(parts.table(k), one.table(k)) for k in range(6))
    one.reset()
    assert not one.summary()[0].any() and not any(one.table(k).any() for k in range(6))
    with pytest.raises(AssertionError):
        qc.Qc(max_cycle=100)


def test_filter_cycles_and_clamps():
    q = qc.Qc(exclude=0x4, max_cycle=64, max_isize=50)
    n = q.add(qrec(16, 0, 0, 255, -1, -1, 0, "70M", [1] * 3 + [2] * 67, [254] * 70) +       # reverse: cycle 0 is the last base, G
              qrec(4, -1, -1, 0, -1, -1, 0, "", "AC", [1, 1]) +                              # excluded here, counted by rule 2
              qrec(0xA3, 0, 9, 7, 0, 5, 60, "10M70D65I", "A" * 75, None))                    # POS > next_pos, forward: outward; clamps
    assert n == 2
    flags, s = q.summary()
    assert flags[0, 0] == 3 and s[0] == 2 and s[1] == 145 and s[9] == 6 + 11 and s[10] == 1 and s[7] == 254 * 64 and s[8] == 64
    assert q.table(qc.RL).reshape(2, 65)[:, 64].tolist() == [1, 1]
    base = q.table(qc.BASE).reshape(2, 64, 5)
    assert base[0, :, 2].sum() == 64 and base[0, 63, 3] == 0 and base[1, :, 0].sum() == 64  # the three A of the reverse record lie past max_cycle
    assert q.table(qc.QUAL).reshape(2, 64, 64)[0, :, 63].sum() == 64
    assert q.table(qc.MAPQ)[[7, 255]].tolist() == [1, 1]
    assert q.table(qc.ISIZE).reshape(3, 51)[1, 50] == 1 and q.insert_size()[0] == 0
    assert q.table(qc.INDEL).reshape(2, 65)[:, 64].tolist() == [1, 1]


GOOD = qrec(0, 0, 5, 60, -1, -1, 0, "3M", "ACG", [30, 30, 30], 0)


def refusals():
    """(tag, records, index of the refused record, reason), each bad record behind good ones"""
    neg = bytearray(qrec(0x904, 0, 5, 60, -1, -1, 0, "", "", []))
    neg[20:24] = struct.pack("<i", -1)                                          # l_seq < 0, in a record the filter would skip
    cig = bytearray(qrec(0x4, 0, 5, 60, -1, -1, 0, "", "", []))
    cig[16:18] = struct.pack("<H", 1)                                           # a CIGAR op with no bytes behind the name
    op = qrec(0x900, 0, 5, 60, -1, -1, 0, [(3, 9)], "", [])                     # op 9, in a record the filter would skip
    short = bytearray(qrec(0x4, 0, 5, 60, -1, -1, 0, "9M", "ACGTACGTA", [30] * 9)[:-3])
    short[0:4] = struct.pack("<I", len(short) - 4)                              # QUAL ends behind the record
    out = [("l_seq", bytes(neg), "bounds"), ("cigar", bytes(cig), "bounds"), ("op", op, "op"), ("qual", bytes(short), "bounds"),
           ("both", qrec(0, 0, 5, 60, -1, -1, 0, [(3, 12)], "ACG", [30] * 3, aux=b"XXq\0"), "op")]      # the op comes first
    for tag, aux in (("type", b"XXq\0"), ("btype", b"XBBA" + struct.pack("<I", 0)), ("bhead", b"XBBc\1\0"),
                     ("brun", b"XBBs" + struct.pack("<I", 3) + b"\0" * 5), ("past", b"XXi\0\0\0"), ("tag", b"XX"), ("nul", b"XXZabc"),
                     ("hnul", b"NMC\3XXH1A")):
        out.append((tag, qrec(0, 0, 5, 60, -1, -1, 0, "3M", "ACG", [30] * 3, aux=aux), "aux"))
    return [(tag, GOOD * k + bad + GOOD, k, why) for k, (tag, bad, why) in enumerate(out, 1)]


@pytest.mark.parametrize("tag,data,at,why", refusals(), ids=[r[0] for r in refusals()])
def test_refusals(tag, data, at, why):
    q = qc.Qc()
    with pytest.raises(qc.QcRefusal) as e:
        q.add(data)
    assert (e.value.record, e.value.why) == (at, why)
    assert not q.summary()[0].any() and not q.summary()[1].any()                # nothing of the call is added
    # the same aux bytes on a record that rule 1 does not walk: unmapped, or filtered out
    if why == "aux":
        rec = bam.split_records(data)[at]
        for flag in (0x4, 0x100):
            ok = bytearray(rec)
            ok[18:20] = struct.pack("<H", flag)
            assert q.add(bytes(ok)) == (1 if flag == 0x4 else 0)


B_ARRAY = b"XBBS" + struct.pack("<I", 2) + b"\1\0\2\0"
OTHERS = (b"XAAx" + aux_int(b"Xc", b"c", -3) + aux_int(b"XC", b"C", 200) + aux_int(b"Xs", b"s", -300) + aux_int(b"XS", b"S", 60000) +
          aux_int(b"Xi", b"i", -70000) + aux_int(b"XI", b"I", 4000000000) + b"Xff" + struct.pack("<f", 1.5) + b"XZZtext\0" + b"XHH1AE3\0" +
          B_ARRAY + b"XbBf" + struct.pack("<If", 1, 2.5) + b"XeBc" + struct.pack("<I", 0))
NM_CASES = [(aux_int(b"NM", t, v), v) for t, v in ((b"c", 7), (b"C", 200), (b"s", 300), (b"S", 60000), (b"i", 70000), (b"I", 3000000000))] + \
           [(OTHERS + aux_int(b"NM", b"C", 9), 9),                              # behind a field of every other type
            (aux_int(b"NM", b"c", -1), None), (aux_int(b"NM", b"i", -5), None), (b"NMZ12\0", None), (OTHERS, None), (b"", None),
            (b"NMZ12\0" + aux_int(b"NM", b"s", -2) + aux_int(b"NM", b"S", 4) + aux_int(b"NM", b"C", 8), 4)]     # the first that qualifies


def test_nm():
    for aux, want in NM_CASES:
        assert qc.walk_aux(aux) == (True, want), aux
        q = qc.Qc()
        assert q.add(qrec(0, 0, 5, 60, -1, -1, 0, "3M", "ACG", [30] * 3, aux=aux)) == 1
        s = q.summary()[1]
        assert (int(s[5]), int(s[6])) == ((want, 0) if want is not None else (0, 1)), aux
    q = qc.Qc()
    q.add(b"".join(qrec(0, 0, 5, 60, -1, -1, 0, "3M", "ACG", [30] * 3, aux=aux) for aux, _ in NM_CASES))
    assert int(q.summary()[1][5]) == sum(v for _, v in NM_CASES if v is not None) and int(q.summary()[1][6]) == 5
