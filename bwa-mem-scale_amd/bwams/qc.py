"""Alignment QC restated in numpy: the yardstick of csrc/qc.hip and host/qc_text.cpp.

The rules are numbered in include/bwams.h above bwams_qc_open; the numbers below are theirs.  Qc(...) accumulates records (BAM
records with their block_size, back to back, as bwams/bam.py builds them) into the flag counters, the scalars and the six tables;
summary, table and text return what the C-ABI's return.
"""
from __future__ import annotations

import math
import struct

import numpy as np

from bwams import bam

DEFAULT_EXCLUDE, DEFAULT_MAX_CYCLE, DEFAULT_MAX_ISIZE = 0x900, 512, 8000
FLAGS = ("total", "primary", "secondary", "supplementary", "duplicates", "primary_duplicates", "mapped", "primary_mapped", "paired",
         "read1", "read2", "properly_paired", "both_mapped", "singletons", "mate_other_ref", "mate_other_ref_mapq5")     # rule 2
SCALARS = ("reads", "bases", "mapped", "bases_mapped", "clipped", "nm_sum", "nm_missing", "qual_sum", "qual_bases", "bases_over",
           "no_qual")                                                                                                  # rule 5
RL, QUAL, BASE, MAPQ, ISIZE, INDEL = range(6)                                                      # bwams_qc_table's `what`
TEXT_FLAGSTAT, TEXT_STATS = 0, 1
FLAGSTAT_LABELS = ("in total (QC-passed reads + QC-failed reads)", "primary", "secondary", "supplementary", "duplicates",
                   "primary duplicates", "mapped", "primary mapped", "paired in sequencing", "read1", "read2", "properly paired",
                   "with itself and mate mapped", "singletons", "with mate mapped to a different chr",
                   "with mate mapped to a different chr (mapQ>=5)")
_PERCENT_OF = {6: 0, 7: 1, 11: 8, 13: 8}                                                           # rule 7: counter -> its denominator
_BASE_OF_CODE = np.full(16, 4, np.int64)                                                           # rule 4c: every code but 1 2 4 8 is N
_BASE_OF_CODE[[1, 2, 4, 8]] = [0, 1, 2, 3]
_AUX_SIZE = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}
_INT_FMT = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}


class QcRefusal(ValueError):
    """Rule 1 (BWAMS_ERR_ARG); .record is the record's index in the call, .why "bounds", "op" or "aux"."""

    def __init__(self, record: int, why: str):
        super().__init__(f"record {record}: {why}")
        self.record, self.why = record, why


def walk_aux(aux: bytes):
    """(ok, NM or None) of one record's aux area: rule 1's walk and rule 5's NM"""
    at, nm = 0, None
    while at < len(aux):
        if at + 3 > len(aux):
            return False, None
        tag, t = aux[at:at + 2], aux[at + 2:at + 3]
        at += 3
        if t in _AUX_SIZE:
            size = _AUX_SIZE[t]
        elif t in (b"Z", b"H"):
            end = aux.find(b"\0", at)
            if end < 0:
                return False, None
            size = end + 1 - at
        elif t == b"B":
            if at + 5 > len(aux) or aux[at:at + 1] not in _AUX_SIZE or aux[at:at + 1] == b"A":
                return False, None
            size = 5 + _AUX_SIZE[aux[at:at + 1]] * struct.unpack_from("<I", aux, at + 1)[0]
        else:
            return False, None
        if at + size > len(aux):
            return False, None
        if nm is None and tag == b"NM" and t in _INT_FMT:
            v = struct.unpack_from(_INT_FMT[t], aux, at)[0]
            if v >= 0:
                nm = v
        at += size
    return True, nm


class Qc:
    def __init__(self, exclude: int = DEFAULT_EXCLUDE, max_cycle: int = DEFAULT_MAX_CYCLE, max_isize: int = DEFAULT_MAX_ISIZE):
        assert max_cycle % 64 == 0 and 64 <= max_cycle <= 4096 and 1 <= max_isize <= 1 << 20 and 0 <= exclude <= 0xFFFF
        self.exclude, self.max_cycle, self.max_isize = exclude, max_cycle, max_isize
        self.reset()

    def reset(self):                                                                               # rule 6
        mc, mi = self.max_cycle, self.max_isize
        self.flags = np.zeros((2, 16), np.int64)
        self.scalars = np.zeros(16, np.int64)
        self.tables = [np.zeros((2, mc + 1), np.int64), np.zeros((2, mc, 64), np.int64), np.zeros((2, mc, 5), np.int64),
                       np.zeros(256, np.int64), np.zeros((3, mi + 1), np.int64), np.zeros((2, 65), np.int64)]

    def add(self, records: bytes) -> int:
        """Every record of `records`; -> the number rule 3's filter let through.  Check first, then add (rule 1)."""
        recs = bam.split_records(records)
        parsed = []
        for k, rec in enumerate(recs):
            refid, pos, l_name, mapq, _bin, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 4)
            cig_at = 36 + l_name
            if l_seq < 0 or cig_at + 4 * n_cig > len(rec):
                raise QcRefusal(k, "bounds")
            cigar = [(c >> 4, c & 15) for c in struct.unpack_from("<%dI" % n_cig, rec, cig_at)]
            if any(op > 8 for _, op in cigar):
                raise QcRefusal(k, "op")
            seq_at = cig_at + 4 * n_cig
            aux_at = seq_at + (l_seq + 1) // 2 + l_seq
            nm = None
            if not flag & self.exclude:
                if aux_at > len(rec):
                    raise QcRefusal(k, "bounds")
                if not flag & 0x4:
                    ok, nm = walk_aux(rec[aux_at:])
                    if not ok:
                        raise QcRefusal(k, "aux")
            parsed.append((rec, refid, pos, mapq, cigar, flag, l_seq, nref, npos, tlen, seq_at, nm))
        n_counted = 0
        S = {n: k for k, n in enumerate(SCALARS)}
        rl, qual_t, base_t, mapq_t, isize_t, indel_t = self.tables
        mc, mi = self.max_cycle, self.max_isize
        for rec, refid, pos, mapq, cigar, flag, l_seq, nref, npos, tlen, seq_at, nm in parsed:
            f = self.flags[1 if flag & 0x200 else 0]                                               # rule 2
            primary, mapped = not flag & 0x900, not flag & 0x4
            f[0] += 1
            f[1] += primary
            f[2] += bool(flag & 0x100)
            f[3] += bool(flag & 0x800) and not flag & 0x100
            f[4] += bool(flag & 0x400)
            f[5] += primary and bool(flag & 0x400)
            f[6] += mapped
            f[7] += primary and mapped
            if primary and flag & 0x1:
                both = not flag & 0xC
                f[8] += 1
                f[9] += bool(flag & 0x40)
                f[10] += bool(flag & 0x80)
                f[11] += bool(flag & 0x2) and mapped
                f[12] += both
                f[13] += bool(flag & 0x8) and mapped
                f[14] += both and nref != refid
                f[15] += both and nref != refid and mapq >= 5
            if flag & self.exclude:                                                                # rule 3
                continue
            n_counted += 1
            cls, rev = (1 if flag & 0x80 else 0), bool(flag & 0x10)
            s = self.scalars
            s[S["reads"]] += 1
            s[S["bases"]] += l_seq
            rl[cls, min(l_seq, mc)] += 1                                                           # rule 4a
            n = min(l_seq, mc)
            s[S["bases_over"]] += l_seq - n
            packed = np.frombuffer(rec, np.uint8, (l_seq + 1) // 2, seq_at)
            codes = np.stack([packed >> 4, packed & 15], 1).reshape(-1)[:l_seq]
            q = np.frombuffer(rec, np.uint8, l_seq, seq_at + (l_seq + 1) // 2).astype(np.int64)
            b = _BASE_OF_CODE[codes]
            if rev:                                                                                # cycles in the read's own direction
                b, q = np.where(b < 4, 3 - b, b)[::-1], q[::-1]
            np.add.at(base_t[cls], (np.arange(n), b[:n]), 1)                                       # rule 4c
            if l_seq > 0 and rec[seq_at + (l_seq + 1) // 2] == 0xFF:
                s[S["no_qual"]] += 1
            elif l_seq > 0:
                np.add.at(qual_t[cls], (np.arange(n), np.minimum(q[:n], 63)), 1)                   # rule 4b
                s[S["qual_sum"]] += int(q[:n].sum())
                s[S["qual_bases"]] += n
            if mapped:
                s[S["mapped"]] += 1
                mapq_t[mapq] += 1                                                                  # rule 4d
                for length, op in cigar:
                    if op in (0, 1, 7, 8):
                        s[S["bases_mapped"]] += length
                    if op == 4:
                        s[S["clipped"]] += length
                    if op in (1, 2) and length >= 1:
                        indel_t[op - 1, min(length, 64)] += 1                                      # rule 4f
                if nm is None:
                    s[S["nm_missing"]] += 1
                else:
                    s[S["nm_sum"]] += nm
            if flag & 0x1 and not flag & 0xC and refid == nref >= 0 and tlen > 0:                  # rule 4e
                if bool(flag & 0x10) == bool(flag & 0x20):
                    row = 2
                else:
                    row = int(rev) if pos <= npos else 1 - int(rev)
                isize_t[row, min(tlen, mi)] += 1
        return n_counted

    def summary(self):
        return self.flags.copy(), self.scalars.copy()

    def table(self, what: int) -> np.ndarray:
        return self.tables[what].reshape(-1).copy()

    def insert_size(self):
        """rule 7: (n, mean, sd, median) over the bins below max_isize of the three rows together; mean and sd are None when n is 0"""
        c = [int(v) for v in self.tables[ISIZE][:, :self.max_isize].sum(0)]
        n = sum(c)
        if n == 0:
            return 0, None, None, 0
        s1, s2 = sum(x * v for x, v in enumerate(c)), sum(x * x * v for x, v in enumerate(c))
        cum, median = 0, 0
        for x, v in enumerate(c):
            cum += v
            if cum >= (n + 1) // 2:
                median = x
                break
        return n, float(s1) / float(n), math.sqrt(float(n * s2 - s1 * s1)) / float(n), median

    def text(self, what: int) -> str:                                                              # rule 7
        if what == TEXT_FLAGSTAT:
            rows = []
            for k, label in enumerate(FLAGSTAT_LABELS):
                a, b = int(self.flags[0, k]), int(self.flags[1, k])
                row = "%d + %d %s" % (a, b, label)
                if k in _PERCENT_OF:
                    d = [int(v) for v in self.flags[:, _PERCENT_OF[k]]]
                    row += " (%s : %s)" % tuple("%.2f%%" % (100.0 * x / y) if y else "N/A" for x, y in zip((a, b), d))
                rows.append(row + "\n")
            return "".join(rows)
        assert what == TEXT_STATS
        s = {n: int(self.scalars[k]) for k, n in enumerate(SCALARS)}
        rows = ["SN\t%s\t%d\n" % (n, s[n]) for n in SCALARS]
        rows.append("SN\terror_rate\t%s\n" % ("%.6e" % (float(s["nm_sum"]) / float(s["bases_mapped"])) if s["bases_mapped"] else "0"))
        rows.append("SN\taverage_quality\t%s\n" % ("%.1f" % (float(s["qual_sum"]) / float(s["qual_bases"])) if s["qual_bases"] else "0"))
        n, mean, sd, median = self.insert_size()
        rows.append("SN\tinsert_size_n\t%d\n" % n)
        rows.append("SN\tinsert_size_mean\t%s\n" % ("%.1f" % mean if n else "0"))
        rows.append("SN\tinsert_size_sd\t%s\n" % ("%.1f" % sd if n else "0"))
        rows.append("SN\tinsert_size_median\t%d\n" % median)
        rl, qual_t, base_t, mapq_t, isize_t, indel_t = self.tables
        for x in np.flatnonzero(rl.any(0)):
            rows.append("RL\t%d\t%d\t%d\n" % (x, rl[0, x], rl[1, x]))
        for tag, t in (("FFQ", qual_t[0]), ("LFQ", qual_t[1])):
            used = np.flatnonzero(t.any(1))
            for c in range(int(used[-1]) + 1 if len(used) else 0):
                rows.append("%s\t%d\t%s\n" % (tag, c + 1, "\t".join(str(int(v)) for v in t[c])))
        used = np.flatnonzero(base_t.any((0, 2)))
        for c in range(int(used[-1]) + 1 if len(used) else 0):
            rows.append("GCC\t%d\t%s\n" % (c + 1, "\t".join(str(int(v)) for v in np.concatenate([base_t[0, c], base_t[1, c]]))))
        for x in np.flatnonzero(mapq_t):
            rows.append("MAPQ\t%d\t%d\n" % (x, mapq_t[x]))
        for x in np.flatnonzero(isize_t.any(0)):
            rows.append("IS\t%d\t%d\t%d\t%d\n" % (x, isize_t[0, x], isize_t[1, x], isize_t[2, x]))
        for x in np.flatnonzero(indel_t.any(0)):
            rows.append("ID\t%d\t%d\t%d\n" % (x, indel_t[0, x], indel_t[1, x]))
        return "".join(rows)
