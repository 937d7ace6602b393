"""The BAI restatement (bwams/bai.py) and the coordinate order (bwams/bam.py: coord_key / coord_sort) on small BAMs made in Python:
records spanning members, a record ending exactly at a member cut, unmapped records placed on a reference, unplaced records, a
reference with no records; every query against brute force."""
import struct

import numpy as np
import pytest

from bwams import bai, bam, bgzf

NAMES = [b"r0", b"r1", b"empty", b"r3"]
LENS = [300000, 70000, 5000, 40000]


def _records(n, seed):
    """SAM lines of n records on NAMES (none on "empty"): mapped with M / D / N / I / S CIGARs (some spanning 16 kb windows),
    unmapped placed at a position, unplaced"""
    rng = np.random.default_rng(seed)
    lines = []
    for i in range(n):
        kind = rng.random()
        nm = b"q%d" % i
        if kind < 0.06:
            lines.append(b"%s\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII" % nm)
            continue
        t = int(rng.choice([0, 1, 3], p=[0.6, 0.25, 0.15]))
        pos = int(rng.integers(1, LENS[t] - 400))
        if kind < 0.15:
            lines.append(b"%s\t%d\t%s\t%d\t0\t*\t=\t%d\t0\tACGTA\tIIIII" % (nm, 4 | 8 * (i & 1), NAMES[t], pos, pos))
            continue
        m = int(rng.integers(20, 120))
        cig = b"%dM" % m
        if kind < 0.25:
            cig = b"5S%dM2I%dM" % (m, int(rng.integers(5, 40)))
        elif kind < 0.32:
            cig = b"%dM%dN%dM" % (m, int(rng.integers(10000, 40000)), int(rng.integers(10, 50)))
            pos = min(pos, LENS[t] - 41000 - m) if LENS[t] > 41000 + m else 1
        elif kind < 0.4:
            cig = b"%dM%dD%dM" % (m, int(rng.integers(1, 30)), int(rng.integers(10, 50)))
        l_seq = sum(int(x) for x, op in bam._CIGAR.findall(cig) if op in b"MIS=X")
        seq = bytes(rng.choice(list(b"ACGT"), l_seq).astype(np.uint8))
        flag = 16 if rng.random() < 0.5 else 0
        lines.append(b"%s\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t%s" % (nm, flag, NAMES[t], pos, cig, seq, b"I" * l_seq))
    ref_id = {n: i for i, n in enumerate(NAMES)}
    return b"".join(bam.encode_record(ln, ref_id, k) for k, ln in enumerate(lines))


def _file(records, block):
    hdr = bam.header_block(b"@HD\tVN:1.6\tSO:coordinate\n", NAMES, LENS)
    return bgzf.compress(hdr + records, 1, block=block), len(hdr)


def _regions(rng, n):
    out = []
    for _ in range(n):
        t = int(rng.integers(0, len(NAMES)))
        a = int(rng.integers(0, LENS[t]))
        out.append((t, a, a + int(rng.choice([1, 50, 2000, 16384, 70000]))))
    for t, ln in enumerate(LENS):
        out.append((t, 0, ln))                                          # whole references
        for w in range(1, ln >> 14):
            out.append((t, (w << 14) - 3, (w << 14) + 3))               # straddling a 16 kb boundary
    return out


def _check_queries(data, records, rng, n=150):
    idx = bai.read(bai.build(data))
    for t, a, b in _regions(rng, n):
        assert bai.query(idx, data, t, a, b) == bai.overlapping(records, t, a, b), (t, a, b)
    return idx


def test_coord_key_and_stable_sort():
    ref_id = {n: i for i, n in enumerate(NAMES)}
    lines = [b"a\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*", b"b\t16\tr1\t5\t0\t3M\t*\t0\t0\tACG\tIII", b"c\t0\tr1\t5\t0\t3M\t*\t0\t0\tACG\tIII",
             b"d\t0\tr0\t9\t0\t3M\t*\t0\t0\tACG\tIII", b"e\t0\tr1\t5\t0\t3M\t*\t0\t0\tACG\tIII", b"f\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*"]
    recs = [bam.encode_record(ln, ref_id) for ln in lines]
    assert bam.coord_key(recs[0]) == 0xFFFFFFFF << 32 and bam.coord_key(recs[1]) == 1 << 32 | 5 << 1 | 1
    got = bam.split_records(bam.coord_sort(b"".join(recs)))
    assert [r[36:37] for r in got] == [b"d", b"c", b"e", b"b", b"a", b"f"]
    assert bam.record_end(recs[1]) == 7 and bam.record_end(recs[0]) == 0


def test_build_and_query_against_brute_force():
    rng = np.random.default_rng(1)
    records = bam.coord_sort(_records(3000, 2))
    data, _ = _file(records, 9000)                                     # many members: records span them
    idx = _check_queries(data, records, rng)
    recs = bam.split_records(records)
    for t in range(len(NAMES)):
        mine = [r for r in recs if struct.unpack_from("<i", r, 4)[0] == t]
        if not mine:
            assert idx["refs"][t]["bins"] == {} and idx["refs"][t]["lin"] == []
            continue
        pseudo = idx["refs"][t]["bins"][bai.PSEUDO_BIN]
        unm = sum(struct.unpack_from("<H", r, 18)[0] & 4 != 0 for r in mine)
        assert pseudo[1] == (len(mine) - unm, unm) and unm > 0
    assert idx["refs"][2]["bins"] == {}                                 # the reference with no records
    assert idx["n_no_coor"] == sum(struct.unpack_from("<i", r, 4)[0] < 0 for r in recs) > 0


def test_record_ending_at_a_member_cut():
    rng = np.random.default_rng(3)
    records = bam.coord_sort(_records(600, 4))
    _, h = _file(b"", 65280)
    ends = np.cumsum([len(r) for r in bam.split_records(records)]) + h
    cut = int(ends[len(ends) // 3])                                    # members of `cut` bytes: a record ends exactly at one
    data, _ = _file(records, cut)
    assert len(bgzf.walk(data)) > 3
    idx = _check_queries(data, records, rng, 80)
    st = bai._Stream(data)                                             # the record ending at the cut ends in the first member's data;
    assert st.voff_end(cut) == st.coff[0] << 16 | cut                  # the next one starts the second member
    assert st.voff_beg(cut) == st.coff[1] << 16
    assert idx["refs"][0]["bins"]


def test_one_member_and_empty():
    rng = np.random.default_rng(5)
    records = bam.coord_sort(_records(200, 6))
    data, _ = _file(records, 65280)
    assert len(bgzf.walk(data)) == 2                                   # one member of records and header, and the EOF member
    _check_queries(data, records, rng, 40)
    data, _ = _file(b"", 65280)
    b = bai.build(data)
    assert b == b"BAI\1" + struct.pack("<i", 4) + struct.pack("<ii", 0, 0) * 4 + struct.pack("<Q", 0)
    assert bai.query(bai.read(b), data, 0, 0, 100) == []


@pytest.mark.parametrize("n", [0, 1])
def test_tiny(n):
    records = bam.coord_sort(_records(n, 7))
    data, _ = _file(records, 65280)
    idx = bai.read(bai.build(data))
    for t, ln in enumerate(LENS):
        assert bai.query(idx, data, t, 0, ln) == bai.overlapping(records, t, 0, ln)
