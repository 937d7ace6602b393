"""BAM records as read input, restated in Python: the yardstick of csrc/bam_reads.hip.

The behaviour is `samtools fastq` (htslib's bam2fq) in front of `bwa mem`; the rules are numbered as in include/bwams.h above
bwams_bam_reads_decode.  reads(records, tags) gives (name, codes, qual | None, comment) per kept read, to_fastq(records, tags) the
equivalent four-line FASTQ text.  BadRecord is the C-ABI's BWAMS_ERR_ARG, Unsupported its BWAMS_ERR_UNSUPPORTED; both carry the
record's ordinal and byte offset.
"""
from __future__ import annotations

import struct

import numpy as np

SKIP_FLAGS = 0x900                               # secondary | supplementary: samtools fastq's default -F
MAX_TAGS = 32
_CODE = np.full(16, 4, np.uint8)                 # rule 3: the 4-bit codes of A, C, G, T; everything else is N
_CODE[[1, 2, 4, 8]] = [0, 1, 2, 3]
_INT = {ord("c"): "<b", ord("C"): "<B", ord("s"): "<h", ord("S"): "<H", ord("i"): "<i", ord("I"): "<I"}
_B_SIZE = {ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4}


class BadRecord(ValueError):
    """Rule 1 (or a malformed aux field, rule 6): BWAMS_ERR_ARG.  .ordinal / .offset name the record."""

    def __init__(self, ordinal: int, offset: int, why: str):
        super().__init__(f"record {ordinal} at byte {offset}: {why}")
        self.ordinal, self.offset = ordinal, offset


class Unsupported(ValueError):
    """Rules 4 and 6: BWAMS_ERR_UNSUPPORTED.  .ordinal / .offset name the record."""

    def __init__(self, ordinal: int, offset: int, why: str):
        super().__init__(f"record {ordinal} at byte {offset}: {why}")
        self.ordinal, self.offset = ordinal, offset


def parse_tags(tags) -> list[bytes]:
    tags = tags or b""
    if len(tags) & 1 or len(tags) > 2 * MAX_TAGS:
        raise ValueError("tags: two-letter tags back to back, at most 32")
    return [bytes(tags[i:i + 2]) for i in range(0, len(tags), 2)]


def record_offsets(records: bytes) -> list[int]:
    """Rule 1: where the records start.  Raises BadRecord for the earliest one that is not well formed."""
    n = len(records)
    out = []
    q = 0
    while q < n:
        k = len(out)
        if q + 36 > n:
            raise BadRecord(k, q, "the buffer ends inside the record")
        (block_size,) = struct.unpack_from("<I", records, q)
        l_name = records[q + 12]
        (n_cig,) = struct.unpack_from("<H", records, q + 16)
        (l_seq,) = struct.unpack_from("<i", records, q + 20)
        if block_size < 32 or l_name < 1 or l_seq < 0:
            raise BadRecord(k, q, "block_size, l_read_name or l_seq")
        if 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > block_size:
            raise BadRecord(k, q, "the fields do not fit block_size")
        if q + 4 + block_size > n:
            raise BadRecord(k, q, "the record ends behind the buffer")
        if records[q + 35 + l_name] != 0:
            raise BadRecord(k, q, "the name does not end in NUL")
        out.append(q)
        q += 4 + block_size
    return out


def _aux_fields(rec: bytes, p: int, k: int, q: int):
    """(position, tag, type, value bytes) of every aux field of the record rec (block_size included) from p on."""
    end = len(rec)
    while p < end:
        if p + 3 > end:
            raise BadRecord(k, q, "an aux field runs past its record")
        tag, ty, v = rec[p:p + 2], rec[p + 2], p + 3
        if ty in (ord("A"), ord("c"), ord("C")):
            e = v + 1
        elif ty in (ord("s"), ord("S")):
            e = v + 2
        elif ty in (ord("i"), ord("I"), ord("f")):
            e = v + 4
        elif ty in (ord("Z"), ord("H")):
            z = rec.find(b"\0", v)
            if z < 0:
                raise BadRecord(k, q, "an aux string without NUL inside its record")
            e = z + 1
        elif ty == ord("B"):
            if v + 5 > end:
                raise BadRecord(k, q, "an aux field runs past its record")
            if rec[v] not in _B_SIZE:
                raise BadRecord(k, q, "a B array of unknown element type")
            e = v + 5 + struct.unpack_from("<I", rec, v + 1)[0] * _B_SIZE[rec[v]]
        else:
            raise BadRecord(k, q, f"an aux field of unknown type {ty!r}")
        if e > end:
            raise BadRecord(k, q, "an aux field runs past its record")
        yield p, tag, ty, rec[v:e]
        p = e


def _comment(rec: bytes, aux_at: int, want: list[bytes], k: int, q: int) -> bytes:
    """Rule 6: every field is walked in record order; the first field of each listed tag is taken, in list order."""
    first = {}
    for _, tag, ty, val in _aux_fields(rec, aux_at, k, q):
        if tag in first or tag not in want:
            continue
        if ty in (ord("f"), ord("B")):
            raise Unsupported(k, q, f"listed tag {tag!r} of type f or B")
        first[tag] = (ty, val)
    out = []
    for tag in want:
        if tag not in first:
            continue
        ty, val = first[tag]
        if ty == ord("A"):
            out.append(tag + b":A:" + val)
        elif ty in (ord("Z"), ord("H")):
            out.append(tag + b":" + bytes([ty]) + b":" + val[:-1])
        else:
            out.append(tag + b":i:%d" % struct.unpack(_INT[ty], val)[0])
    return b"\t".join(out)


def reads(records: bytes, tags=b""):
    """The kept reads of BAM records (no header block): [(name, codes uint8, qual bytes | None, comment bytes)].  Qualities are
    None for every read when no kept record has any."""
    want = parse_tags(tags)
    out = []
    first_qual = None                                 # (has qualities, ordinal) of the first kept record
    for k, q in enumerate(record_offsets(records)):
        (block_size,) = struct.unpack_from("<I", records, q)
        rec = records[q:q + 4 + block_size]
        l_name = rec[12]
        n_cig, flag, l_seq = struct.unpack_from("<HHi", rec, 16)
        if flag & SKIP_FLAGS:
            continue
        if l_seq == 0:
            raise Unsupported(k, q, "a read without bases")
        seq_at = 36 + l_name + 4 * n_cig
        qual_at = seq_at + (l_seq + 1) // 2
        aux_at = qual_at + l_seq
        has_q = rec[qual_at] != 0xFF
        if first_qual is None:
            first_qual = (has_q, k)
        elif has_q != first_qual[0]:
            raise Unsupported(k, q, f"qualities {'present' if has_q else 'absent'}, unlike record {first_qual[1]}")
        packed = np.frombuffer(rec, np.uint8, (l_seq + 1) // 2, seq_at)
        nib = np.stack([packed >> 4, packed & 15], 1).reshape(-1)[:l_seq]
        codes = _CODE[nib]
        qual = np.frombuffer(rec, np.uint8, l_seq, qual_at)
        if flag & 0x10:
            codes = np.where(codes < 4, 3 - codes, 4).astype(np.uint8)[::-1]
            qual = qual[::-1]
        comment = _comment(rec, aux_at, want, k, q) if want else b""
        out.append((rec[36:36 + l_name - 1], np.ascontiguousarray(codes), bytes((qual + 33).astype(np.uint8)) if has_q else None, comment))
    return out


def to_fastq(records: bytes, tags=b"") -> bytes:
    """The FASTQ text `samtools fastq -T tags` would write, without its "/1" and "/2" (FASTA text when there are no qualities)."""
    out = []
    for name, codes, qual, comment in reads(records, tags):
        head = name + (b" " + comment if comment else b"")
        seq = bytes(b"ACGTN"[c] for c in codes)
        out.append(b"@" + head + b"\n" + seq + b"\n+\n" + qual + b"\n" if qual is not None else b">" + head + b"\n" + seq + b"\n")
    return b"".join(out)


def count(records: bytes) -> tuple[int, int, int]:
    """(records, kept reads, bases of the kept reads), as bwams_bam_reads_decode and the BAM reader count them."""
    offs = record_offsets(records)
    kept = [q for q in offs if not struct.unpack_from("<H", records, q + 18)[0] & SKIP_FLAGS]
    return len(offs), len(kept), sum(struct.unpack_from("<i", records, q + 20)[0] for q in kept)
