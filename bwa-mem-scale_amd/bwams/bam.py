"""BAM (SAMv1 §4.2) restated in Python: the yardstick of csrc/bam.hip.

encode_records(sam_text, ref_names) turns SAM lines into BAM alignment records with htslib's rules (sam_parse1 + bam_write1),
refusing what csrc/bam.hip refuses (BamRefusal, with the line's index); header_block(text, names, lengths) is the header block;
decode(bam_bytes) reads an uncompressed BAM stream (header block and records) back, records as SAM lines.  coord_key / coord_sort
restate the coordinate order of csrc/bam_sort.hip (samtools sort's default), record_end the end its coords carry.
"""
from __future__ import annotations

import re
import struct

import numpy as np

NT16 = b"=ACMGRSVTWYHKDBN"
CIGAR_OPS = b"MIDNSHP=X"
_NT16_CODE = {c: i for i, c in enumerate(NT16)}
_INT = re.compile(rb"[-+]?[0-9]{1,18}\Z")
_FLOAT = re.compile(rb"[-+]?([0-9]+\.?[0-9]*|\.[0-9]+)\Z")
_CIGAR = re.compile(rb"([0-9]+)([MIDNSHP=X])")


class BamRefusal(ValueError):
    """A line BAM cannot hold (csrc/bam.hip's BWAMS_ERR_UNSUPPORTED); .line is its index in the text."""

    def __init__(self, line: int, why: str):
        super().__init__(f"line {line}: {why}")
        self.line = line


def reg2bin(beg: int, end: int) -> int:
    """SAMv1 §5.3: the bin of [beg, end)."""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def int_type(x: int) -> tuple[bytes, bytes]:
    """htslib's smallest type of an 'i' value: (type char, little-endian bytes)."""
    if x < 0:
        for t, f, lo in ((b"c", "<b", -128), (b"s", "<h", -32768), (b"i", "<i", -(1 << 31))):
            if x >= lo:
                return t, struct.pack(f, x)
    else:
        for t, f, hi in ((b"C", "<B", 255), (b"S", "<H", 65535), (b"I", "<I", (1 << 32) - 1)):
            if x <= hi:
                return t, struct.pack(f, x)
    raise OverflowError(x)


def _num(field: bytes, lo: int, hi: int, line: int) -> int:
    if not _INT.match(field) or not lo <= int(field) <= hi:
        raise BamRefusal(line, f"bad number {field!r}")
    return int(field)


def _aux(f: bytes, line: int) -> bytes:
    if len(f) < 5 or f[2:3] != b":" or f[4:5] != b":":
        raise BamRefusal(line, f"not a TG:T:value field: {f!r}")
    tag, ty, v = f[:2], f[3:4], f[5:]
    if ty == b"A":
        if len(v) != 1:
            raise BamRefusal(line, f"A field of {len(v)} characters")
        return tag + b"A" + v
    if ty == b"i":
        if not _INT.match(v):
            raise BamRefusal(line, f"bad integer {f!r}")
        x = int(v)
        if not -(1 << 31) <= x <= (1 << 32) - 1:
            raise BamRefusal(line, f"integer outside int32 / uint32: {f!r}")
        t, b = int_type(x)
        return tag + t + b
    if ty == b"f":
        if not _FLOAT.match(v) or sum(c in b"0123456789" for c in v) > 15:
            raise BamRefusal(line, f"bad float {f!r}")
        return tag + b"f" + np.float32(float(v)).tobytes()
    if ty in (b"Z", b"H"):
        return tag + ty + v + b"\0"
    raise BamRefusal(line, f"type {ty!r} (B arrays are not supported)")


def encode_record(line: bytes, ref_id: dict, k: int = 0) -> bytes:
    """One SAM line (without its newline) as one BAM record (block_size included)."""
    f = line.split(b"\t")
    if len(f) < 11:
        raise BamRefusal(k, "fewer than 11 fields")
    name = f[0]
    if len(name) < 1:
        raise BamRefusal(k, "empty read name")
    if len(name) > 254:
        raise BamRefusal(k, "read name longer than 254 bytes")
    flag = _num(f[1], 0, 0xFFFF, k)
    pos = _num(f[3], 0, 0x7FFFFFFF, k) - 1
    mapq = _num(f[4], 0, 255, k)
    pnext = _num(f[7], 0, 0x7FFFFFFF, k) - 1
    tlen = _num(f[8], -(1 << 31), (1 << 31) - 1, k)

    def rid(x):
        if x == b"*":
            return -1
        if x not in ref_id:
            raise BamRefusal(k, f"unknown reference {x!r}")
        return ref_id[x]

    refid = rid(f[2])
    nrefid = refid if f[6] == b"=" else rid(f[6])
    cig = []
    if f[5] != b"*":
        ops = _CIGAR.findall(f[5])
        if not ops or b"".join(a + b for a, b in ops) != f[5] or any(int(a) >= 1 << 28 for a, _ in ops):
            raise BamRefusal(k, f"bad CIGAR {f[5][:40]!r}")
        if len(ops) > 0xFFFF:
            raise BamRefusal(k, "more than 65535 CIGAR operations")
        cig = [(int(a), CIGAR_OPS.index(b)) for a, b in ops]
    rlen = sum(n for n, op in cig if op in (0, 2, 3, 7, 8))
    end = pos + 1 if (flag & 4) or not cig or rlen == 0 else pos + rlen
    seq = b"" if f[9] == b"*" else f[9]
    if f[10] != b"*" and len(f[10]) != len(seq):
        raise BamRefusal(k, "SEQ and QUAL of different lengths")
    codes = [_NT16_CODE.get(c, 15) for c in seq] + [0]
    packed = bytes(codes[i] << 4 | (codes[i + 1] if i + 1 < len(seq) else 0) for i in range(0, len(seq), 2))
    qual = b"\xff" * len(seq) if f[10] == b"*" else bytes(c - 33 & 0xFF for c in f[10])
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(name) + 1, mapq, reg2bin(pos, end), len(cig), flag, len(seq), nrefid,
                       pnext, tlen)
    body += name + b"\0" + b"".join(struct.pack("<I", n << 4 | op) for n, op in cig) + packed + qual
    body += b"".join(_aux(a, k) for a in f[11:])
    return struct.pack("<I", len(body)) + body


def encode_records(sam_text: bytes, ref_names) -> bytes:
    """Every line of sam_text (each ending in a newline) as one BAM record, in order; ref_names in the index's order."""
    ref_id = {(n if isinstance(n, bytes) else n.encode()): i for i, n in enumerate(ref_names)}
    lines = sam_text.split(b"\n")
    assert lines[-1] == b"", "SAM text ends with a newline"
    return b"".join(encode_record(ln, ref_id, k) for k, ln in enumerate(lines[:-1]))


def header_block(text: bytes, names, lengths) -> bytes:
    """The BAM header block: magic, l_text, text, n_ref, then l_name / name + NUL / l_ref per reference."""
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(names))
    for n, ln in zip(names, lengths):
        n = n if isinstance(n, bytes) else n.encode()
        out += struct.pack("<i", len(n) + 1) + n + b"\0" + struct.pack("<i", ln)
    return out


def _fmt_float(x: float) -> bytes:
    return b"%g" % x


def decode_record(rec: bytes, names) -> bytes:
    """One BAM record (without block_size) back as a SAM line (no newline); floats printed with %g."""
    (refid, pos, l_name, mapq, _bin, n_cig, flag, l_seq, nrefid, pnext, tlen) = struct.unpack_from("<iiBBHHHiiii", rec, 0)
    p = 32
    name = rec[p:p + l_name - 1]
    p += l_name
    cig = b"".join(b"%d%c" % (c >> 4, CIGAR_OPS[c & 15]) for c in struct.unpack_from("<%dI" % n_cig, rec, p)) or b"*"
    p += 4 * n_cig
    nb = (l_seq + 1) // 2
    seq = bytes(NT16[(rec[p + i // 2] >> (4 * (1 - i % 2))) & 15] for i in range(l_seq)) or b"*"
    p += nb
    q = rec[p:p + l_seq]
    qual = b"*" if l_seq == 0 or q[:1] == b"\xff" else bytes(c + 33 for c in q)
    p += l_seq
    rname = b"*" if refid < 0 else names[refid]
    rnext = b"*" if nrefid < 0 else b"=" if nrefid == refid else names[nrefid]
    f = [name, b"%d" % flag, rname, b"%d" % (pos + 1), b"%d" % mapq, cig, rnext, b"%d" % (pnext + 1), b"%d" % tlen, seq, qual]
    fmt = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}
    while p < len(rec):
        tag, ty = rec[p:p + 2], rec[p + 2:p + 3]
        p += 3
        if ty == b"A":
            f.append(tag + b":A:" + rec[p:p + 1]); p += 1
        elif ty in fmt:
            (x,) = struct.unpack_from(fmt[ty], rec, p)
            f.append(tag + b":i:%d" % x); p += struct.calcsize(fmt[ty])
        elif ty == b"f":
            (x,) = struct.unpack_from("<f", rec, p)
            f.append(tag + b":f:" + _fmt_float(x)); p += 4
        elif ty in (b"Z", b"H"):
            e = rec.index(b"\0", p)
            f.append(tag + b":" + ty + b":" + rec[p:e]); p = e + 1
        else:
            raise ValueError(f"aux type {ty!r}")
    return b"\t".join(f)


def split_records(data: bytes, p: int = 0) -> list[bytes]:
    """The records (block_size included) of data[p:]."""
    out = []
    while p < len(data):
        (bs,) = struct.unpack_from("<I", data, p)
        out.append(data[p:p + 4 + bs])
        p += 4 + bs
    assert p == len(data), "truncated record"
    return out


def record_end(rec: bytes) -> int:
    """The end reg2bin takes of one record (block_size included): POS + the CIGAR's reference length (M/D/N/=/X), or POS + 1 when
    unmapped, without CIGAR or of reference length 0 — wrapped to int32, as bwams_bam_coord_t.end holds it."""
    (pos, l_name, n_cig, flag) = struct.unpack_from("<iBxxxHH", rec, 8)
    ops = struct.unpack_from("<%dI" % n_cig, rec, 36 + l_name)
    rlen = sum(c >> 4 for c in ops if c & 15 in (0, 2, 3, 7, 8))
    end = pos + 1 if (flag & 4) or not ops or rlen == 0 else pos + rlen
    return (end + (1 << 31)) % (1 << 32) - (1 << 31)


def coord_key(rec: bytes) -> int:
    """The coordinate order's key of one record (block_size included): (uint32)refID << 32 | (uint32)(POS + 1) << 1 | reverse
    strand — samtools sort's default order, refID -1 (unplaced) last.  include/bwams_types.h (bwams_bam_coord_t) defines it."""
    (refid, pos, flag) = struct.unpack_from("<ii6xH", rec, 4)
    return (refid & 0xFFFFFFFF) << 32 | ((pos + 1) & 0xFFFFFFFF) << 1 | (flag >> 4 & 1)


def coord_sort(records: bytes) -> bytes:
    """The records of `records` (block_size included, back to back) in coordinate order: a stable sort by coord_key."""
    recs = split_records(records)
    return b"".join(sorted(recs, key=coord_key))


def decode(bam_bytes: bytes, names=None):
    """An uncompressed BAM stream -> (header text, [(name, length)], SAM text of the records).  Without the magic, bam_bytes is
    records only and names the references."""
    refs = []
    text = b""
    p = 0
    if bam_bytes[:4] == b"BAM\1":
        (l_text,) = struct.unpack_from("<i", bam_bytes, 4)
        text = bam_bytes[8:8 + l_text]
        p = 8 + l_text
        (n_ref,) = struct.unpack_from("<i", bam_bytes, p)
        p += 4
        for _ in range(n_ref):
            (ln,) = struct.unpack_from("<i", bam_bytes, p)
            nm = bam_bytes[p + 4:p + 4 + ln - 1]
            (lr,) = struct.unpack_from("<i", bam_bytes, p + 4 + ln)
            refs.append((nm, lr))
            p += 8 + ln
        names = [n for n, _ in refs]
    names = [(n if isinstance(n, bytes) else n.encode()) for n in (names or [])]
    sam = b"".join(decode_record(r[4:], names) + b"\n" for r in split_records(bam_bytes, p))
    return text, refs, sam
