"""Depth of coverage restated in numpy: the yardstick of csrc/depth.hip and host/depth_text.cpp.

The rules are numbered in include/bwams.h above bwams_depth_open; the numbers below are theirs.  Depth(l_ref, ...) accumulates
records (BAM records with their block_size, back to back, as bwams/bam.py builds them), finish() turns the counters into depths, and
the queries return what the C-ABI's return: summary rows, histograms, window sums, runs, and the three texts.
"""
from __future__ import annotations

import struct

import numpy as np

from bwams import bam

DEFAULT_EXCLUDE = 0x704
TEXT_SUMMARY, TEXT_DIST, TEXT_WINDOWS = 0, 1, 2


class DepthRefusal(ValueError):
    """Rule 3: a record with an op code above 8 (BWAMS_ERR_ARG); .record is its index in the call."""

    def __init__(self, record: int):
        super().__init__(f"record {record} has a CIGAR op code above 8")
        self.record = record


def fields(rec: bytes):
    """(refID, POS, MAPQ, FLAG, [(length, op)]) of one record (block_size included)."""
    refid, pos, l_name, mapq, _bin, n_cig, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    ops = struct.unpack_from("<%dI" % n_cig, rec, 36 + l_name)
    return refid, pos, mapq, flag, [(c >> 4, c & 15) for c in ops]


def stretches(pos: int, cigar, count_deletions: bool):
    """Rule 3 before clipping: the covered stretches [a, b) of a CIGAR walked from pos; ops that touch on the reference merge."""
    out = []
    x = pos
    open_ = False
    for n, op in cigar:
        if op in (0, 7, 8) or (op == 2 and count_deletions):
            if open_:
                out[-1][1] = x + n
            else:
                out.append([x, x + n])
                open_ = True
            x += n
        elif op in (2, 3):                                    # a gap: the next covering op starts a new stretch
            x += n
            open_ = False
    return [tuple(s) for s in out if s[1] > s[0]]


class Depth:
    def __init__(self, l_ref, exclude: int = DEFAULT_EXCLUDE, min_mapq: int = 0, count_deletions: bool = False):
        self.l_ref = [int(x) for x in l_ref]
        assert all(x >= 0 for x in self.l_ref)                                # rule 1
        self.exclude, self.min_mapq, self.count_deletions = exclude, min_mapq, bool(count_deletions)
        self.reset()

    def reset(self):                                                          # rule 6
        self.diff = [np.zeros(n + 1, np.int64) for n in self.l_ref]
        self.depth = None

    def counts(self, refid, mapq, flag, cigar) -> bool:                       # rule 2
        return not flag & self.exclude and mapq >= self.min_mapq and 0 <= refid < len(self.l_ref) and len(cigar) > 0

    def add(self, records: bytes) -> int:
        """Every record of `records`; -> the number that counted.  Check first, then add (rule 3)."""
        assert self.depth is None, "rule 6: no add after finish"
        recs = [fields(r) for r in bam.split_records(records)]
        for k, (_, _, _, _, cigar) in enumerate(recs):
            if any(op > 8 for _, op in cigar):
                raise DepthRefusal(k)
        n = 0
        for refid, pos, mapq, flag, cigar in recs:
            if not self.counts(refid, mapq, flag, cigar):
                continue
            n += 1
            ln = self.l_ref[refid]
            for a, b in stretches(pos, cigar, self.count_deletions):
                a, b = max(a, 0), min(b, ln)                                  # clipped, not refused
                if a < b:
                    self.diff[refid][a] += 1
                    self.diff[refid][b] -= 1
        return n

    def finish(self):                                                         # rule 6
        if self.depth is None:
            self.depth = [np.cumsum(d)[:-1] for d in self.diff]
        return self

    def summary(self):                                                        # rule 7
        return [dict(length=len(d), bases=int(d.sum()), min=int(d.min()) if len(d) else 0, max=int(d.max()) if len(d) else 0)
                for d in self.depth]

    def hist(self, ref: int, n_bins: int) -> np.ndarray:                      # rule 8
        assert 2 <= n_bins <= 1 << 20 and -1 <= ref < len(self.l_ref)
        d = np.concatenate(self.depth + [np.zeros(0, np.int64)]) if ref < 0 else self.depth[ref]
        return np.bincount(np.minimum(d, n_bins - 1), minlength=n_bins).astype(np.int64)

    def windows(self, w: int) -> np.ndarray:                                  # rule 9
        assert w >= 1
        out = [np.add.reduceat(d, np.arange(0, len(d), w)) for d in self.depth if len(d)]
        return np.concatenate(out + [np.zeros(0, np.int64)]).astype(np.int64)

    def runs(self, ref: int, beg: int, end: int):                             # rule 10
        d = self.depth[ref][beg:end]
        if len(d) == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        first = np.flatnonzero(np.concatenate([[True], d[1:] != d[:-1]]))
        return (first + beg).astype(np.int32), d[first].astype(np.int32)

    def text(self, names, what: int, arg: int = 0) -> str:                    # rule 11
        names = [n.decode() if isinstance(n, bytes) else n for n in names]
        rows = self.summary()
        if what == TEXT_SUMMARY:
            def line(name, r):
                mean = r["bases"] / r["length"] if r["length"] else 0.0
                return "%s\t%d\t%d\t%.2f\t%d\t%d\n" % (name, r["length"], r["bases"], mean, r["min"], r["max"])
            some = [r for r in rows if r["length"] > 0]
            total = dict(length=sum(r["length"] for r in rows), bases=sum(r["bases"] for r in rows),
                         min=min((r["min"] for r in some), default=0), max=max((r["max"] for r in some), default=0))
            return "chrom\tlength\tbases\tmean\tmin\tmax\n" + "".join(line(n, r) for n, r in zip(names, rows)) + line("total", total)
        if what == TEXT_DIST:
            n_bins = arg or 1024

            def block(name, h):
                total, out, above = int(h.sum()), [], 0
                occupied = np.flatnonzero(h)
                for v in range(int(occupied[-1]) if len(occupied) else -1, -1, -1):
                    above += int(h[v])
                    out.append("%s\t%d\t%.4f\n" % (name, v, above / total))
                return "".join(out)
            return block("total", self.hist(-1, n_bins)) + "".join(block(n, self.hist(r, n_bins)) for r, n in enumerate(names))
        if what == TEXT_WINDOWS:
            sums, out, k = self.windows(arg), [], 0
            for n, ln in zip(names, self.l_ref):
                for beg in range(0, ln, arg):
                    end = min(beg + arg, ln)
                    out.append("%s\t%d\t%d\t%.2f\n" % (n, beg, end, int(sums[k]) / (end - beg)))
                    k += 1
            return "".join(out)
        raise ValueError(what)
