"""Inputs shared by tests/test_gunzip.py (CPU) and tests/test_gpu_gunzip.py: gzip files of every shape, made with zlib."""
import struct
import zlib

import numpy as np


def fastq_text(n, seed=0, read_len=150):
    """n FASTQ records of fixed shape, as tests/test_gpu_inflate.py builds them (the same bytes for the same arguments)."""
    rng = np.random.default_rng(seed)
    name = np.frombuffer(b"".join(b"@r%09d\n" % i for i in range(n)), np.uint8).reshape(n, 12)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, read_len))]
    seq[rng.random((n, read_len)) < 0.002] = ord("N")
    qual = (rng.integers(0, 41, (n, read_len)) + 33).astype(np.uint8)
    nl = np.full((n, 1), 10, np.uint8)
    plus = np.frombuffer(b"+\n", np.uint8)[None, :].repeat(n, 0)
    return np.concatenate([name, seq, nl, plus, qual, nl], axis=1).tobytes()


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush=zlib.Z_SYNC_FLUSH, mem_level=8):
    """A raw DEFLATE stream of data; flush_at: offsets at which the compressor is flushed (sync or full)."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    parts, at = [], 0
    for f in flush_at:
        parts += [c.compress(data[at:f]), c.flush(flush)]
        at = f
    parts += [c.compress(data[at:]), c.flush()]
    return b"".join(parts)


def member(data, level=6, fname=None, fextra=None, fcomment=None, fhcrc=False, raw=None, **kw):
    """One gzip member of data, its header fields made by hand.  raw: the DEFLATE stream to use instead of compressing."""
    flg = (4 if fextra is not None else 0) | (8 if fname is not None else 0) | (16 if fcomment is not None else 0) | (2 if fhcrc else 0)
    h = struct.pack("<BBBBIBB", 31, 139, 8, flg, 0, 0, 255)
    if fextra is not None:
        h += struct.pack("<H", len(fextra)) + fextra
    if fname is not None:
        h += fname + b"\0"
    if fcomment is not None:
        h += fcomment + b"\0"
    if fhcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xffff)
    body = raw if raw is not None else raw_deflate(data, level, **kw)
    return h + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def marker_text(n=700, back=80, run=2_200_000, seed=11):
    """(text, flush offsets).  Records whose name and sequence lines repeat those of `back` records (some 25 KB) earlier while the
    quality lines are random, so most of a piece's symbols refer to bytes in front of it; then a run of one byte, flushed every
    16 KiB so that block starts lie inside it; then more records."""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        if i < back:
            nm = b"@INSTR:%04d:FLOWCELLX:%d:%05d:%05d 1:N:0:ACGTAC" % (i, i % 8, int(rng.integers(0, 99999)), int(rng.integers(0, 99999)))
            sq = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 150)])
        else:
            nm, sq = recs[i - back][0], recs[i - back][1]
        recs.append((nm, sq, bytes((rng.integers(0, 41, 150) + 33).astype(np.uint8))))
    lines = [b"%s\n%s\n+\n%s\n" % r for r in recs]
    head, tail = b"".join(lines[:n - 100]), b"".join(lines[n - 100:])
    text = head + b"A" * run + tail
    return text, list(range(len(head) + 16384, len(head) + run, 16384))
