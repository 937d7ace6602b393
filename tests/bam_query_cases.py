"""Builders shared by test_bam_query_plan.py and test_gpu_bam_query.py: small coordinate-sorted BAM files made in Python
(bwams.bam.encode_record, bwams.bgzf.compress, bwams.bai.build), the named cases of a region query with their region lists, and
the brute-force answer of a query (bwams.bai.overlapping per region, united by record)."""
import struct

import numpy as np

from bwams import bai, bam, bgzf

NAMES = [b"big", b"mid", b"empty"]
LENS = [9000000, 200000, 50000]                  # "big" crosses 2^23, so a record on it can sit in a level-1 bin
REF_ID = {n: i for i, n in enumerate(NAMES)}
HEADER_TEXT = b"@HD\tVN:1.6\tSO:coordinate\n"


def line(name: bytes, ref: int, pos0: int, cigar: bytes, flag: int = 0, rng=None, aux=()) -> bytes:
    """One SAM line; pos0 is 0-based; the bases and qualities (2 to 74) are random when rng is given"""
    l_seq = sum(int(x) for x, op in bam._CIGAR.findall(cigar) if op in b"MIS=X") if cigar != b"*" else 40
    seq = bytes(rng.choice(list(b"ACGT"), l_seq).astype(np.uint8)) if rng is not None else b"ACGT" * (l_seq // 4) + b"ACGT"[:l_seq % 4]
    rname = NAMES[ref] if ref >= 0 else b"*"
    qual = bytes((rng.integers(2, 75, l_seq) + 33).astype(np.uint8)) if rng is not None else b"I" * l_seq
    return b"\t".join([name, b"%d" % flag, rname, b"%d" % (pos0 + 1), b"60", cigar, b"*", b"0", b"0", seq, qual] + list(aux))


def encode(lines) -> bytes:
    """The lines as BAM records in coordinate order (stable)"""
    return bam.coord_sort(b"".join(bam.encode_record(ln, REF_ID, k) for k, ln in enumerate(lines)))


def bam_file(records: bytes, block: int) -> bytes:
    return bgzf.compress(bam.header_block(HEADER_TEXT, NAMES, LENS) + records, 1, block=block)


def background(rng, n: int, tag: bytes = b"bg", unplaced: int = 0, refs=(0, 1), hi1: int = 0):
    """n records of 40 to 150 bases on `refs` (none on "empty" unless asked; on "mid" below hi1 when given), half of them
    reverse, some with D / I / S ops or placed unmapped, and `unplaced` records without a reference"""
    out = []
    for i in range(n):
        t = int(rng.choice(refs))
        hi = 300000 if t == 0 else (hi1 if t == 1 and hi1 else LENS[t] - 400)
        pos = int(rng.integers(0, hi))
        m = int(rng.integers(40, 151))
        kind = rng.random()
        cig, flag = b"%dM" % m, (16 if rng.random() < 0.5 else 0)
        if kind < 0.1:
            cig = b"5S%dM2I%dM" % (m - 30, 23)
        elif kind < 0.2:
            cig = b"%dM%dD%dM" % (m - 20, int(rng.integers(1, 30)), 20)
        elif kind < 0.25:
            cig, flag = b"*", 4
        out.append(line(b"%s%d" % (tag, i), t, pos, cig, flag, rng))
    out += [line(b"%su%d" % (tag, i), -1, -1, b"*", 4, rng) for i in range(unplaced)]
    return out


# ---- the named cases: one file, a region list each ----
R_N = (0, 100000, 100200)                        # reached by a 70 kb N op that starts four 16 kb windows earlier
R_L1 = (0, 8388650, 8388700)                     # reached by a record that crosses 2^23: bin 1, a level-1 bin
R_EDGE = (1, 5000, 5100)                         # the four edge records and the placed unmapped read


def named_lines(rng):
    return [
        line(b"n70k", 0, 100050 - 70030, b"20M70000N30M", 0, rng),          # [30020, 100070): ends inside R_N
        line(b"lvl1", 0, 8388508, b"100M100N100M", 16, rng),                # [8388508, 8388808): over 2^23
        line(b"end_eq_beg", 1, 4950, b"50M", 0, rng),                       # ends at 5000: out
        line(b"end_beg1", 1, 4951, b"50M", 0, rng),                         # ends at 5001: in
        line(b"pos_end1", 1, 5099, b"40M", 0, rng),                         # POS = end - 1: in
        line(b"pos_end", 1, 5100, b"40M", 0, rng),                          # POS = end: out
        line(b"placed_unmapped", 1, 5050, b"*", 4, rng),                    # end = POS + 1: in
    ]


REGION_LISTS = {
    "n_op_from_another_window": [R_N],
    "level1_bin": [R_L1],
    "edges_and_placed_unmapped": [R_EDGE],
    "behind_last_window": [(1, 199000, 199900)],
    "reference_without_records": [(2, 0, 50000)],
    "overlapping_pair": [(0, 100000, 100200), (0, 100100, 100900)],
    "adjacent_pair": [(1, 4000, 5000), (1, 5000, 5100)],
    "reverse_order": [R_EDGE, R_L1, R_N],
    "whole_references": [(0, 0, LENS[0]), (1, 0, LENS[1])],
    "keeps_none": [(0, 8000000, 8000001)],
}


def named_records(seed: int = 11, n_background: int = 293, unplaced: int = 4) -> bytes:
    """About 300 records: the named ones among background records that end by 120 kb on "mid" (so that its linear index stops far
    in front of 199000) and by 300 kb on "big" """
    rng = np.random.default_rng(seed)
    return encode(named_lines(rng) + background(rng, n_background, unplaced=unplaced, hi1=120000))


def brute(records: bytes, regions) -> list[bytes]:
    """The union, each record once and in file order, of bai.overlapping per region (record names are unique, so records are)"""
    want = set()
    for ref, beg, end in regions:
        want.update(bai.overlapping(records, ref, beg, end))
    return [r for r in bam.split_records(records) if r in want]


def coords_of(recs) -> np.ndarray:
    """(key, end, size) rows as bwams_bam_coord_t holds them"""
    out = np.zeros(len(recs), np.dtype([("key", "<u8"), ("end", "<i4"), ("size", "<i4")]))
    for k, r in enumerate(recs):
        out[k] = (bam.coord_key(r), bam.record_end(r), len(r))
    return out


def random_regions(rng, n: int):
    out = []
    for _ in range(n):
        t = int(rng.integers(0, 3))
        hi = 310000 if t == 0 else LENS[t]
        a = int(rng.integers(0, hi))
        out.append((t, a, a + int(rng.choice([1, 50, 2000, 16384, 70000]))))
    return out


def unique_names(records: bytes) -> bool:
    names = [r[36:36 + r[12]] for r in bam.split_records(records)]
    return len(set(names)) == len(names)


def header_len() -> int:
    return len(bam.header_block(HEADER_TEXT, NAMES, LENS))


def ref_ids(recs):
    return [struct.unpack_from("<i", r, 4)[0] for r in recs]
