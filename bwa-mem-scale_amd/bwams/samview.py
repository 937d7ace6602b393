"""BAM records viewed as SAM text: rules V1-V7 of include/bwams.h (above bwams_samview_open) restated in Python, as the yardstick of
csrc/samview.hip.  The rules are SAMv1 sections 1.4 and 4.2 and htslib's sam_format1; nothing here was run against htslib.

format_record(rec, names) is one record's line; view(records, names, ...) the text and line offsets of an add under rule V2's
filter; check(records, n_ref) rule V6's first refusal; fmt_g(x) rule V5 through the C library's "%g".  Complete for B arrays,
which bwams/bam.py's decode_record is not.
"""
from __future__ import annotations

import struct

import numpy as np

NT16 = b"=ACMGRSVTWYHKDBN"
CIGAR_OPS = b"MIDNSHP=X"
_INT = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}
_SIZE = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}

REASONS = {1: "refID or next refID outside [-1, n_ref)",
           2: "l_read_name is 0, the name does not end in NUL, or it holds a NUL",
           3: "a CIGAR op code above 8",
           4: "l_seq < 0, or the name, CIGAR, SEQ and QUAL pass the record's end",
           5: "the aux fields do not chain to the record's end"}


def fmt_g(x) -> bytes:
    """Rule V5: C's "%g" of the float widened to double.  Python's own "%g" is the C library's but for a NaN's sign, which it drops
    and glibc prints."""
    x = np.float32(x)
    if np.isnan(x):
        return b"-nan" if np.signbit(x) else b"nan"
    return b"%g" % float(x)


def split(records: bytes) -> list[bytes]:
    """The records (block_size included) of a well-formed chain."""
    out, p = [], 0
    while p < len(records):
        (bs,) = struct.unpack_from("<I", records, p)
        out.append(records[p:p + 4 + bs])
        p += 4 + bs
    assert p == len(records), "truncated record"
    return out


def _fixed(rec: bytes):
    return struct.unpack_from("<iiBBHHHiiii", rec, 4)


def _value(ty: bytes, rec: bytes, p: int) -> bytes:
    if ty == b"A":
        return rec[p:p + 1]
    if ty == b"f":
        return fmt_g(struct.unpack_from("<f", rec, p)[0])
    return b"%d" % struct.unpack_from(_INT[ty], rec, p)


def _aux_walk(rec: bytes, a: int):
    """The aux fields of rec from offset a as (tag, type, start, end) with end behind the field, or None when they do not chain to
    the record's end (rule V6.5, the walk of csrc/aux_rg.h).  For Z and H, [start, end - 1) is the value; for B, start is the subtype."""
    n, out = len(rec), []
    while a < n:
        if a + 3 > n:
            return None
        tag, ty = rec[a:a + 2], rec[a + 2:a + 3]
        a += 3
        if ty in (b"Z", b"H"):
            e = rec.find(b"\0", a)
            if e < 0:
                return None
            out.append((tag, ty, a, e + 1))
            a = e + 1
        elif ty == b"B":
            if a + 5 > n:
                return None
            sub = rec[a:a + 1]
            if sub not in _SIZE or sub == b"A":
                return None
            (cnt,) = struct.unpack_from("<I", rec, a + 1)
            e = a + 5 + _SIZE[sub] * cnt
            if e > n:
                return None
            out.append((tag, ty, a, e))
            a = e
        else:
            if ty not in _SIZE or a + _SIZE[ty] > n:
                return None
            out.append((tag, ty, a, a + _SIZE[ty]))
            a += _SIZE[ty]
    return out


def check_record(rec: bytes, n_ref: int):
    """Rule V6 for one record (block_size included): its reason 1-5, the first that holds in the order 1, 4, 2, 3, 5, or None."""
    (refid, _pos, l_name, _mapq, _bin, n_cig, _flag, l_seq, nrefid, _pnext, _tlen) = _fixed(rec)
    n = len(rec)
    if not (-1 <= refid < n_ref and -1 <= nrefid < n_ref):
        return 1
    if l_seq < 0 or 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > n:
        return 4
    name = rec[36:36 + l_name]
    if l_name == 0 or name[-1:] != b"\0" or b"\0" in name[:-1]:
        return 2
    if any(c & 15 > 8 for c in struct.unpack_from("<%dI" % n_cig, rec, 36 + l_name)):
        return 3
    if _aux_walk(rec, 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq) is None:
        return 5
    return None


def check(records, n_ref: int):
    """Rule V6 over an add: (the smallest ordinal with a fault, its reason's text), or None.  records: bytes or a list of records."""
    recs = split(records) if isinstance(records, (bytes, bytearray)) else records
    for k, rec in enumerate(recs):
        why = check_record(rec, n_ref)
        if why:
            return k, REASONS[why]
    return None


def format_record(rec: bytes, names) -> bytes:
    """One record (block_size included) that check_record passes, as its SAM line with the newline: rules V3-V5 and V7."""
    (refid, pos, l_name, mapq, _bin, n_cig, flag, l_seq, nrefid, pnext, tlen) = _fixed(rec)
    p = 36
    name = rec[p:p + l_name - 1]
    p += l_name
    cig = b"".join(b"%d%c" % (c >> 4, CIGAR_OPS[c & 15]) for c in struct.unpack_from("<%dI" % n_cig, rec, p)) or b"*"
    p += 4 * n_cig
    packed = np.frombuffer(rec, np.uint8, (l_seq + 1) // 2, p)
    codes = np.stack([packed >> 4, packed & 15], 1).reshape(-1)[:l_seq]
    seq = np.frombuffer(NT16, np.uint8)[codes].tobytes() or b"*"
    p += (l_seq + 1) // 2
    q = np.frombuffer(rec, np.uint8, l_seq, p)
    qual = b"*" if l_seq == 0 or q[0] == 0xFF else (q + np.uint8(33)).tobytes()
    p += l_seq
    rname = b"*" if refid < 0 else names[refid]
    rnext = b"*" if nrefid < 0 else b"=" if nrefid == refid else names[nrefid]
    f = [name, b"%d" % flag, rname, b"%d" % (pos + 1), b"%d" % mapq, cig, rnext, b"%d" % (pnext + 1), b"%d" % tlen, seq, qual]
    for tag, ty, a, e in _aux_walk(rec, p):
        if ty in (b"Z", b"H"):
            f.append(tag + b":" + ty + b":" + rec[a:e - 1])
        elif ty == b"B":
            sub = rec[a:a + 1]
            (cnt,) = struct.unpack_from("<I", rec, a + 1)
            f.append(tag + b":B:" + sub + b"".join(b"," + _value(sub, rec, a + 5 + _SIZE[sub] * k) for k in range(cnt)))
        else:
            f.append(tag + b":" + (ty if ty in (b"A", b"f") else b"i") + b":" + _value(ty, rec, a))
    return b"\t".join(f) + b"\n"


def keeps(rec: bytes, require: int = 0, exclude: int = 0, min_mapq: int = 0) -> bool:
    """Rule V2."""
    flag, mapq = struct.unpack_from("<H", rec, 18)[0], rec[13]
    return (flag & require) == require and (flag & exclude) == 0 and mapq >= min_mapq


class Refused(ValueError):
    """Rule V6; .ordinal and .reason."""

    def __init__(self, ordinal: int, reason: str):
        super().__init__(f"record {ordinal}: {reason}")
        self.ordinal, self.reason = ordinal, reason


def view(records, names, require: int = 0, exclude: int = 0, min_mapq: int = 0):
    """An add (rules V1, V2, V6): -> (text, line_off: int64[n_lines + 1]).  records: bytes or a list of records; names: the
    references' names as bytes.  Raises Refused, filtered records checked too."""
    recs = split(records) if isinstance(records, (bytes, bytearray)) else records
    bad = check(recs, len(names))
    if bad:
        raise Refused(*bad)
    lines = [format_record(r, names) for r in recs if keeps(r, require, exclude, min_mapq)]
    off = np.zeros(len(lines) + 1, np.int64)
    if lines:
        off[1:] = np.cumsum([len(ln) for ln in lines])
    return b"".join(lines), off


def header_names(block: bytes) -> list[bytes]:
    """The reference names of a BAM header block."""
    (l_text,) = struct.unpack_from("<i", block, 4)
    p = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", block, p)
    p += 4
    names = []
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", block, p)
        names.append(block[p + 4:p + 4 + ln - 1])
        p += 8 + ln
    return names
