"""BAI (SAMv1 §5.2) restated in Python: the yardstick of the index host/bam_sort.cpp writes beside a coordinate-sorted BAM.

build(bam_file) makes the index of a BGZF-compressed, coordinate-sorted BAM file byte for byte as bwams_sorter_close writes it;
read(bai) parses an index; query(index, bam_file, tid, beg, end) returns the records the index's candidate chunks yield that overlap
[beg, end) — what a region query of a BAM reader returns; plan(index, regions) is the plan of such a query over several regions as
bwams_bam_file_query makes it and bwams_bai_plan returns it (host/bam_query.cpp), walk(plan, bam_file, regions) the records it yields.

The rules of a region query (include/bwams.h, "BAM file by region"):
  1. a record overlaps region (ref, beg, end) when refID == ref, POS < end and bam.record_end > beg (overlapping);
  2. regions (0 <= ref < n_ref, 0 <= beg < end, any order, overlapping or not) are sorted by (ref, beg) and merged per reference
     where they overlap or touch; a record that overlaps several comes back once, and records come back in file order;
  3. the plan: for every merged region the chunks of reg2bins(beg, end) — levels the coordinate overruns give no bin, pseudo-bin
     37450 is never a source — that end past the linear index's offset of beg's 16 kb window (the window index clamped to the last
     entry, an empty linear index gives 0), each start clipped to that offset; all of them sorted by virtual offset, and those that
     touch or overlap merged into disjoint intervals;
  4. no regions: the whole file, one interval from the first record to the end of the data, unplaced records included;
  5. a chain of records starts at an interval's start and stops at its end offset.

The rules (htslib's hts_idx_push / hts_idx_finish, with the choices spelled out):
  * a record's span is [max(POS, 0), max(end, that + 1)), end = bam.record_end; its bin is reg2bin of the span;
  * per reference, one chunk [start of the first record, end of the last record) for every stretch of consecutive records of one
    bin; a chunk that starts in the compressed block where its bin's previous chunk ends is merged into it;
  * the 16 kb linear index holds the start of the first record, placed (mapped or not), that covers each window; empty windows in
    front of the first record take the reference's first offset, later ones their left neighbour's;
  * pseudo-bin 37450: (first start, last end), (n_mapped, n_unmapped) — unmapped = FLAG 0x4;
  * bins in ascending order (37450 last); a reference without records has no bins and no linear index; n_no_coor closes the file.
Virtual offsets: a record starting at uncompressed byte x is at (file offset of the member holding x) << 16 | offset in it; one
ending before byte y at (file offset of the member holding y - 1) << 16 | (offset of y - 1 in it) + 1.
"""
from __future__ import annotations

import bisect
import struct
import zlib

from . import bam, bgzf

PSEUDO_BIN = 37450


def reg2bins(beg: int, end: int) -> list[int]:
    """SAMv1 §5.3: every bin that may hold a record overlapping [beg, end)."""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


class _Stream:
    """A BGZF file inflated, with the member bookkeeping that virtual offsets need."""

    def __init__(self, buf: bytes):
        parts, self.coff, self.ustart = [], [], []
        at = 0
        for p, hdr, total, _, isize in bgzf.walk(buf):
            if isize:
                self.coff.append(p)
                self.ustart.append(at)
                parts.append(zlib.decompress(buf[p + hdr:p + total - 8], -15))
            at += isize
        self.data = b"".join(parts)
        self.by_coff = dict(zip(self.coff, self.ustart))

    def voff_beg(self, x: int) -> int:
        i = bisect.bisect_right(self.ustart, x) - 1
        return self.coff[i] << 16 | (x - self.ustart[i])

    def voff_end(self, y: int) -> int:
        i = bisect.bisect_right(self.ustart, y - 1) - 1
        return self.coff[i] << 16 | (y - self.ustart[i])

    def at(self, voff: int) -> int:
        """the uncompressed offset of a virtual offset"""
        return self.by_coff[voff >> 16] + (voff & 0xFFFF)


def _header(data: bytes) -> tuple[int, int]:
    """(n_ref, offset of the first record) of an uncompressed BAM stream"""
    assert data[:4] == b"BAM\1"
    (l_text,) = struct.unpack_from("<i", data, 4)
    p = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", data, p)
    p += 4
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", data, p)
        p += 8 + ln
    return n_ref, p


def _records(data: bytes, p: int):
    """(start, end, record bytes) of every record from p on"""
    while p < len(data):
        (bs,) = struct.unpack_from("<I", data, p)
        yield p, p + 4 + bs, data[p:p + 4 + bs]
        p += 4 + bs


def span(rec: bytes) -> tuple[int, int, int, int]:
    """(refID, POS, the span's beg, the span's end) of a record as the index sees it"""
    refid, pos = struct.unpack_from("<ii", rec, 4)
    beg = max(pos, 0)
    return refid, pos, beg, max(bam.record_end(rec), beg + 1)


def build(bam_file: bytes) -> bytes:
    """The index of a coordinate-sorted BGZF BAM file, as bwams_sorter_close writes <path>.bai."""
    st = _Stream(bam_file)
    n_ref, p0 = _header(st.data)
    refs = [None] * n_ref
    n_no_coor = 0
    cur, chunk = -1, None                     # the reference being indexed; its open chunk [bin, beg, end]

    def add(r, bin_, b, e):
        v = r["bins"].setdefault(bin_, [])
        if v and b >> 16 <= v[-1][1] >> 16:
            v[-1][1] = max(v[-1][1], e)
        else:
            v.append([b, e])

    def end_ref():
        nonlocal cur, chunk
        if cur >= 0 and chunk is not None:
            add(refs[cur], *chunk)
        cur, chunk = -1, None

    for x, y, rec in _records(st.data, p0):
        refid, _, beg, end = span(rec)
        (flag,) = struct.unpack_from("<H", rec, 18)
        if refid < 0:
            end_ref()
            n_no_coor += 1
            continue
        if refid != cur:
            end_ref()
            cur = refid
        r = refs[refid]
        vb, ve = st.voff_beg(x), st.voff_end(y)
        if r is None:
            r = refs[refid] = {"bins": {}, "lin": [], "beg": vb, "end": ve, "mapped": 0, "unmapped": 0}
        r["end"] = ve
        r["unmapped" if flag & 4 else "mapped"] += 1
        b = bam.reg2bin(beg, end)
        if chunk is not None and chunk[0] == b:
            chunk[2] = ve
        else:
            if chunk is not None:
                add(r, *chunk)
            chunk = [b, vb, ve]
        lin = r["lin"]
        w1 = (end - 1) >> 14
        if len(lin) <= w1:
            lin += [None] * (w1 + 1 - len(lin))
        for w in range(beg >> 14, w1 + 1):
            if lin[w] is None:
                lin[w] = vb
    end_ref()
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    for r in refs:
        if r is None:
            out.append(struct.pack("<ii", 0, 0))
            continue
        out.append(struct.pack("<i", len(r["bins"]) + 1))
        for b in sorted(r["bins"]):
            ch = r["bins"][b]
            out.append(struct.pack("<Ii", b, len(ch)) + b"".join(struct.pack("<QQ", *c) for c in ch))
        out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, r["beg"], r["end"], r["mapped"], r["unmapped"]))
        lin, prev = r["lin"], r["beg"]
        for w in range(len(lin)):
            if lin[w] is None:
                lin[w] = prev
            prev = lin[w]
        out.append(struct.pack("<i", len(lin)) + b"".join(struct.pack("<Q", v) for v in lin))
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def read(bai: bytes) -> dict:
    """{"refs": [{"bins": {bin: [(beg, end), ...]}, "lin": [...]}, ...], "n_no_coor": n}; the pseudo-bin stays among the bins"""
    assert bai[:4] == b"BAI\1"
    (n_ref,) = struct.unpack_from("<i", bai, 4)
    p, refs = 8, []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", bai, p)
        p += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, p)
            p += 8
            bins[b] = [struct.unpack_from("<QQ", bai, p + 16 * k) for k in range(n_chunk)]
            p += 16 * n_chunk
        (n_intv,) = struct.unpack_from("<i", bai, p)
        p += 4
        refs.append({"bins": bins, "lin": list(struct.unpack_from("<%dQ" % n_intv, bai, p))})
        p += 8 * n_intv
    n_no_coor = struct.unpack_from("<Q", bai, p)[0] if p + 8 <= len(bai) else None
    return {"refs": refs, "n_no_coor": n_no_coor}


def query(index: dict, bam_file: bytes, tid: int, beg: int, end: int) -> list[bytes]:
    """The records of reference tid overlapping [beg, end) (span end > beg and POS < end) that the index's candidate chunks hold:
    chunks of reg2bins(beg, end) ending past the linear index's offset of beg's window, read in file order."""
    r = index["refs"][tid]
    lin = r["lin"]
    min_off = 0 if not lin else lin[min(beg >> 14, len(lin) - 1)]
    chunks = sorted(c for b in reg2bins(beg, end) if b != PSEUDO_BIN for c in r["bins"].get(b, ()) if c[1] > min_off)
    st = _Stream(bam_file)
    out, seen = [], set()
    for cb, ce in chunks:
        x, stop = st.at(max(cb, min_off)), st.at(ce)
        while x < stop:
            (bs,) = struct.unpack_from("<I", st.data, x)
            rec = st.data[x:x + 4 + bs]
            refid, pos = struct.unpack_from("<ii", rec, 4)
            if refid != tid or pos >= end:
                break
            if bam.record_end(rec) > beg and x not in seen:
                seen.add(x)
                out.append((x, rec))
            x += 4 + bs
    return [rec for _, rec in sorted(out)]


def overlapping(records: bytes, tid: int, beg: int, end: int) -> list[bytes]:
    """Brute force: the records (block_size included, back to back) of tid with POS < end and end > beg, in their order."""
    out = []
    for rec in bam.split_records(records):
        refid, pos = struct.unpack_from("<ii", rec, 4)
        if refid == tid and pos < end and bam.record_end(rec) > beg:
            out.append(rec)
    return out


def merge_regions(regions) -> list[tuple[int, int, int]]:
    """Rule 2: the regions sorted by (ref, beg) and merged per reference where they overlap or touch."""
    out = []
    for ref, beg, end in sorted((int(r), int(b), int(e)) for r, b, e in regions):
        assert ref >= 0 and 0 <= beg < end, (ref, beg, end)
        if out and out[-1][0] == ref and beg <= out[-1][2]:
            out[-1][2] = max(out[-1][2], end)
        else:
            out.append([ref, beg, end])
    return [tuple(x) for x in out]


def _bins(beg: int, end: int):
    """reg2bins(beg, end) with every level clipped to its own bins (a coordinate of 2^29 or more overruns the scheme)"""
    yield 0
    for shift, first, nxt in ((26, 1, 9), (23, 9, 73), (20, 73, 585), (17, 585, 4681), (14, 4681, 37449)):
        yield from range(first + (beg >> shift), min(first + ((end - 1) >> shift), nxt - 1) + 1)


def plan(index: dict, regions) -> list[tuple[int, int]]:
    """Rule 3: the disjoint intervals (beg, end) of virtual offsets, ascending, that hold every record overlapping a region."""
    chunks = []
    for ref, beg, end in merge_regions(regions):
        r = index["refs"][ref]
        lin = r["lin"]
        min_off = 0 if not lin else lin[min(beg >> 14, len(lin) - 1)]
        for b in _bins(beg, end):
            for cb, ce in r["bins"].get(b, ()):
                if ce > min_off and max(cb, min_off) < ce:
                    chunks.append((max(cb, min_off), ce))
    out = []
    for cb, ce in sorted(chunks):
        if out and cb <= out[-1][1]:
            out[-1][1] = max(out[-1][1], ce)
        else:
            out.append([cb, ce])
    return [tuple(c) for c in out]


def walk(intervals, bam_file: bytes, regions) -> list[bytes]:
    """The records a reader gets from a plan: every interval's chain from its start to its end offset, rule 1 against the regions."""
    st = _Stream(bam_file)
    merged = merge_regions(regions)
    out = []
    for vb, ve in intervals:
        x, stop = st.at(vb), st.at(ve)
        while x < stop:
            (bs,) = struct.unpack_from("<I", st.data, x)
            rec = st.data[x:x + 4 + bs]
            refid, pos = struct.unpack_from("<ii", rec, 4)
            if any(refid == ref and pos < end and bam.record_end(rec) > beg for ref, beg, end in merged):
                out.append(rec)
            x += 4 + bs
    return out
