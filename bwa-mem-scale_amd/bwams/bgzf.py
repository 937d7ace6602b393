"""BGZF (SAMv1 §4.1), the blocked gzip that bgzip writes: a writer and a header walker in pure Python.

Test and tool infrastructure for the device inflater (csrc/inflate.hip): the writer makes members of every DEFLATE block kind with
zlib, and the walker lists what the host side of the inflater reads from the header chain.
"""
from __future__ import annotations

import struct
import zlib

BLOCK = 65280                    # input bytes per member, as bgzip cuts them (its compressed size must stay <= 65536)
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def member(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, mem_level: int = 8, flush_at=()) -> bytes:
    """One BGZF member holding `data` (<= 65536 bytes).  flush_at: offsets in `data` at which a Z_SYNC_FLUSH ends the DEFLATE block
    (an empty stored block follows it), so one member holds several blocks."""
    assert len(data) <= 65536
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    parts, at = [], 0
    for f in sorted(flush_at):
        parts.append(c.compress(data[at:f]))
        parts.append(c.flush(zlib.Z_SYNC_FLUSH))
        at = f
    parts.append(c.compress(data[at:]))
    parts.append(c.flush(zlib.Z_FINISH))
    body = b"".join(parts)
    bsize = 12 + 6 + len(body) + 8 - 1
    if bsize > 65535:
        raise ValueError("member does not fit BSIZE (compressed size over 64 KiB)")
    hdr = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, ord("B"), ord("C"), 2, bsize)
    return hdr + body + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


def compress(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, mem_level: int = 8, block: int = BLOCK,
             flush_every: int = 0, eof: bool = True) -> bytes:
    """`data` as BGZF: members of `block` input bytes, each with a sync flush every `flush_every` bytes (0: none), then the EOF member."""
    out = []
    for a in range(0, len(data), block):
        d = data[a:a + block]
        fl = range(flush_every, len(d), flush_every) if flush_every else ()
        out.append(member(d, level, strategy, mem_level, fl))
    if eof:
        out.append(EOF_MEMBER)
    return b"".join(out)


def walk(buf: bytes):
    """The member list of a BGZF buffer: (offset, header bytes, BSIZE + 1, CRC32, ISIZE) per member.  Raises ValueError on a header
    that is not BGZF or a member cut off by the end."""
    out, p = [], 0
    while p < len(buf):
        if len(buf) - p < 18 or buf[p:p + 4] != b"\x1f\x8b\x08\x04":
            raise ValueError(f"no BGZF header at byte {p}")
        xlen = struct.unpack_from("<H", buf, p + 10)[0]
        q, bsize = p + 12, None
        while q + 4 <= p + 12 + xlen:
            si1, si2, slen = buf[q], buf[q + 1], struct.unpack_from("<H", buf, q + 2)[0]
            if si1 == ord("B") and si2 == ord("C") and slen == 2:
                bsize = struct.unpack_from("<H", buf, q + 4)[0]
            q += 4 + slen
        if bsize is None:
            raise ValueError(f"no BC subfield in the header at byte {p}")
        total = bsize + 1
        if p + total > len(buf):
            raise ValueError(f"member at byte {p} is cut off")
        crc, isize = struct.unpack_from("<II", buf, p + total - 8)
        out.append((p, 12 + xlen, total, crc, isize))
        p += total
    return out


def first_block_header(mem: bytes, hdr: int = 18):
    """(BFINAL, BTYPE) of a member's first DEFLATE block: the first 3 bits of its DEFLATE data (BTYPE 0 stored, 1 fixed,
    2 dynamic; BFINAL 0: more blocks follow)."""
    b = mem[hdr]
    return b & 1, (b >> 1) & 3
