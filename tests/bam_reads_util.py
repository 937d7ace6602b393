"""Builders shared by test_bam_reads.py and test_gpu_bam_reads.py: BAM records from bwams.bam.encode_record, and what a read of
such a record must come out as, worked out from the letters (not through bwams.bam_reads)."""
import struct

import numpy as np

from bwams import bam

NT16 = bam.NT16                                   # b"=ACMGRSVTWYHKDBN": letter k is the 4-bit code k
_LETTER = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}


def rec(name: bytes, flag: int = 4, seq: bytes = b"ACGT", qual=None, aux=(), cigar: bytes = b"*", raw_aux: bytes = b"") -> bytes:
    """One BAM record (block_size included).  qual: phred + 33 text or None; aux: SAM fields (b"RG:Z:x"); raw_aux: bytes appended
    behind them as they are (types bam.encode_record does not write)."""
    line = b"\t".join([name, b"%d" % flag, b"*", b"0", b"0", cigar, b"*", b"0", b"0", seq or b"*", b"*" if qual is None else qual] + list(aux))
    r = bam.encode_record(line, {})
    if raw_aux:
        r = struct.pack("<I", len(r) - 4 + len(raw_aux)) + r[4:] + raw_aux
    return r


def read_of(name: bytes, flag: int, seq: bytes, qual, comment: bytes = b""):
    """(name, codes, qual, comment) the record rec(name, flag, seq, qual) stands for"""
    codes = np.array([_LETTER.get(c, 4) for c in seq], np.uint8)
    if flag & 0x10:
        codes = np.array([3 - c if c < 4 else 4 for c in codes[::-1]], np.uint8)
        qual = qual[::-1] if qual is not None else None
    return name, codes, qual, comment


def same_reads(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and np.array_equal(g[1], w[1]) and g[2] == w[2] and g[3] == w[3], (k, g, w)


def rand_seq(rng, n: int, letters: bytes = b"ACGTN") -> bytes:
    return bytes(np.frombuffer(letters, np.uint8)[rng.integers(0, len(letters), n)])


def rand_qual(rng, n: int) -> bytes:
    return bytes((rng.integers(0, 42, n) + 33).astype(np.uint8))


def fetched(f):
    """capi.Fastq.fetch() in the shape of bam_reads.reads()"""
    d = f.fetch()
    q = bytes(d["quals"]) if d["quals"] is not None else None
    cum = d["cum"]
    return [(d["names"][k], d["enc"][cum[k]:cum[k + 1]], q[cum[k]:cum[k + 1]] if q is not None else None, d["comments"][k] or b"")
            for k in range(d["n"])]


def many_records(n: int, seed: int):
    """n records with l_seq 30..300, names of varied length, some reverse, some secondary / supplementary, some aux — built with
    numpy and struct (encode_record per record would take the test's seconds).  Returns (records, expected reads for tags RGNM)."""
    rng = np.random.default_rng(seed)
    l_seq = rng.integers(30, 301, n)
    flags = np.where(rng.random(n) < 0.3, 0x10, 0) | np.where(rng.random(n) < 0.05, 0x100, 0) | np.where(rng.random(n) < 0.03, 0x800, 0)
    nib = rng.choice(np.array([1, 2, 4, 8, 15], np.uint8), int(l_seq.sum()), p=[0.24, 0.24, 0.24, 0.24, 0.04])
    quals = rng.integers(0, 42, int(l_seq.sum())).astype(np.uint8)
    code = np.full(16, 4, np.uint8)
    code[[1, 2, 4, 8]] = [0, 1, 2, 3]
    out, want = [], []
    at = 0
    for k in range(n):
        l = int(l_seq[k])
        name = b"r%d" % k + b"x" * (k % 23)
        nb, q = nib[at:at + l], quals[at:at + l]
        at += l
        pk = np.zeros((l + 1) // 2 * 2, np.uint8)
        pk[:l] = nb
        packed = (pk[0::2] << 4 | pk[1::2]).tobytes()
        aux = b""
        comment = []
        if k % 3 == 0:
            aux += b"NMC" + bytes([k % 200])
            comment.append(b"NM:i:%d" % (k % 200))
        if k % 4 == 0:
            aux = b"RGZ" + b"g%d\0" % (k % 7) + aux
            comment.insert(0, b"RG:Z:g%d" % (k % 7))
        n_cig = k % 3
        body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 0, 4680, n_cig, int(flags[k]), l, -1, -1, 0) + name + b"\0" + \
            struct.pack("<%dI" % n_cig, *([l << 4] * n_cig)) + packed + q.tobytes() + aux
        out.append(struct.pack("<I", len(body)) + body)
        if not flags[k] & 0x900:
            c, qq = code[nb], q + 33
            if flags[k] & 0x10:
                c, qq = np.where(c < 4, 3 - c, 4).astype(np.uint8)[::-1], qq[::-1]
            want.append((name, c, qq.astype(np.uint8).tobytes(), b"\t".join(comment)))
    return b"".join(out), want
