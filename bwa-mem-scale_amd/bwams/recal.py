"""Base recalibration tables restated in numpy: the yardstick of csrc/recal.hip and host/recal_text.cpp.

The rules are numbered in include/bwams.h above bwams_recal_open; the numbers below are theirs.  Recal(l_ref, rg_ids, ...) holds the
reference codes and known flags per position and the four tables; add() takes BAM records with their block_size, back to back, as
bwams/bam.py builds them.  All four tables are counted independently per base (the device folds QUAL and RG from CYCLE).
"""
from __future__ import annotations

import numpy as np

from bwams import bam, markdup
from bwams.pileup import fields

DEFAULT_EXCLUDE = 0x704
RG, QUAL, CYCLE, CONTEXT = range(4)
N_QUAL = 94
_BASE_OF_CODE = np.full(16, -1, np.int64)                                                # rules 6 and 7: the codes 1 2 4 8 are A C G T
_BASE_OF_CODE[[1, 2, 4, 8]] = [0, 1, 2, 3]
_REF_OPS, _QUERY_OPS = (0, 2, 3, 7, 8), (0, 1, 4, 7, 8)


class RecalRefusal(ValueError):
    """Rule 5 (BWAMS_ERR_ARG); .record is the record's index in the call, .why "op", "bounds", "length", "cycle" or "aux"."""

    def __init__(self, record: int, why: str):
        super().__init__(f"record {record}: {why}")
        self.record, self.why = record, why


class Recal:
    def __init__(self, l_ref, rg_ids=None, exclude: int = DEFAULT_EXCLUDE, min_mapq: int = 1, min_baseq: int = 6, max_cycle: int = 500):
        assert exclude <= 0xFFFF and 0 <= min_baseq <= 93 and max_cycle >= 1                     # rule 1
        self.l_ref = [int(x) for x in l_ref]
        self.rg_ids = None if rg_ids is None else [x if isinstance(x, bytes) else x.encode() for x in rg_ids]
        self.n_rg = 0 if rg_ids is None else len(self.rg_ids)
        self.exclude, self.min_mapq, self.min_baseq, self.max_cycle = exclude, min_mapq, min_baseq, max_cycle
        self.ref = [np.full(n, 4, np.uint8) for n in self.l_ref]                                 # rule 2
        self.known = [np.zeros(n, bool) for n in self.l_ref]                                     # rule 3
        self.n_bases = 0
        self.reset()

    def reset(self):                                                                             # rule 3: the reference and the flags stay
        g = self.n_rg + 1
        self.tables = [np.zeros((g, 2), np.int64), np.zeros((g, N_QUAL, 2), np.int64),
                       np.zeros((g, N_QUAL, 2 * self.max_cycle + 1, 2), np.int64), np.zeros((g, N_QUAL, 16, 2), np.int64)]

    def table(self, what: int) -> np.ndarray:
        return self.tables[what]

    def set_ref(self, ref: int, codes):                                                          # rule 2
        codes = np.asarray(codes, np.uint8)
        assert len(codes) == self.l_ref[ref] and (codes <= 4).all()
        self.ref[ref] = codes.copy()

    def add_known(self, sites):                                                                  # rule 3: all checked, then all set
        sites = [tuple(int(v) for v in s) for s in sites]
        for k, (r, b, e) in enumerate(sites):
            if not (0 <= r < len(self.l_ref) and 0 <= b < e <= self.l_ref[r]):
                raise ValueError("interval %d" % k)
        for r, b, e in sites:
            self.known[r][b:e] = True

    def counts_head(self, refid, mapq, flag, cigar, l_seq) -> bool:                              # rule 4 without the QUAL byte
        return not flag & self.exclude and mapq >= self.min_mapq and 0 <= refid < len(self.l_ref) and len(cigar) > 0 and l_seq > 0

    def group(self, rec: bytes) -> int:                                                          # rule 6
        if self.rg_ids is None:
            return 0
        v = markdup.read_group(rec)
        return self.rg_ids.index(v) if v in self.rg_ids else self.n_rg

    def add(self, records: bytes) -> int:
        """Every record of `records`; -> the number that counted.  Check first, then add (rule 5)."""
        raw = bam.split_records(records)
        recs = [fields(r) for r in raw]
        counted = []
        for k, (refid, _, mapq, flag, cigar, l_seq, codes, qual) in enumerate(recs):
            if any(op > 8 for _, op in cigar):
                raise RecalRefusal(k, "op")
            if not self.counts_head(refid, mapq, flag, cigar, l_seq):
                continue
            if len(codes) != l_seq:                                                              # SEQ or QUAL ends behind the record
                raise RecalRefusal(k, "bounds")
            if qual[0] == 0xFF:
                continue
            if sum(n for n, op in cigar if op in _QUERY_OPS) != l_seq:
                raise RecalRefusal(k, "length")
            if l_seq > self.max_cycle:
                raise RecalRefusal(k, "cycle")
            if self.rg_ids is not None:
                try:
                    markdup.read_group(raw[k])
                except ValueError:
                    raise RecalRefusal(k, "aux") from None
            counted.append(k)
        self.n_bases = 0
        for k in counted:
            refid, pos, _, flag, cigar, l_seq, codes, qual = recs[k]
            g = self.group(raw[k])
            rev, neg = bool(flag & 0x10), flag & 0x81 == 0x81
            i = np.arange(l_seq)
            cyc = (l_seq - i if rev else i + 1) * (-1 if neg else 1)
            base = _BASE_OF_CODE[codes]
            nb = np.full(l_seq, -1, np.int64)                                                    # the neighbour in sequencing order
            if rev:
                nb[:-1] = base[1:]
                ctx = np.where((nb >= 0) & (base >= 0), 4 * (3 - nb) + (3 - base), -1)
            else:
                nb[1:] = base[:-1]
                ctx = np.where((nb >= 0) & (base >= 0), 4 * nb + base, -1)
            x = np.full(l_seq, -1, np.int64)                                                     # the position of a base in M, = or X
            at, q = pos, 0
            for n, op in cigar:
                if op in (0, 7, 8):
                    x[q:q + n] = np.maximum(np.arange(at, at + n), -1)
                if op in _REF_OPS:
                    at += n
                if op in _QUERY_OPS:
                    q += n
            ok = (x >= 0) & (x < self.l_ref[refid]) & (base >= 0) & (qual >= self.min_baseq)     # rule 7
            xi = np.where(ok, x, 0)
            if self.l_ref[refid] == 0:
                continue
            ok &= (self.ref[refid][xi] < 4) & ~self.known[refid][xi]
            err = (self.ref[refid][xi] != base).astype(np.int64)
            qq = np.minimum(qual.astype(np.int64), N_QUAL - 1)
            sel = np.flatnonzero(ok)
            add = np.stack([np.ones(len(sel), np.int64), err[sel]], 1)                           # (observation, error) per base
            self.tables[RG][g] += add.sum(0)
            np.add.at(self.tables[QUAL][g], qq[sel], add)
            np.add.at(self.tables[CYCLE][g], (qq[sel], cyc[sel] + self.max_cycle), add)
            has = ctx[sel] >= 0                                                                  # rule 7: no context, no CONTEXT count
            np.add.at(self.tables[CONTEXT][g], (qq[sel][has], ctx[sel][has]), add[has])
            self.n_bases += len(sel)
        return len(counted)

    def text(self) -> str:                                                                       # rule 10
        ids = [x.decode("latin-1") for x in (self.rg_ids or [])] + ["*"]
        rows = []
        t = self.tables
        for g in np.flatnonzero(t[RG][:, 0] > 0):
            rows.append("RG\t%s\t%d\t%d\n" % (ids[g], t[RG][g, 0], t[RG][g, 1]))
        for g, q in np.argwhere(t[QUAL][:, :, 0] > 0):
            rows.append("QUAL\t%s\t%d\t%d\t%d\n" % (ids[g], q, t[QUAL][g, q, 0], t[QUAL][g, q, 1]))
        for g, q, c in np.argwhere(t[CYCLE][:, :, :, 0] > 0):
            rows.append("CYCLE\t%s\t%d\t%d\t%d\t%d\n" % (ids[g], q, c - self.max_cycle, t[CYCLE][g, q, c, 0], t[CYCLE][g, q, c, 1]))
        for g, q, c in np.argwhere(t[CONTEXT][:, :, :, 0] > 0):
            rows.append("CONTEXT\t%s\t%d\t%s%s\t%d\t%d\n" % (ids[g], q, "ACGT"[c >> 2], "ACGT"[c & 3], t[CONTEXT][g, q, c, 0],
                                                             t[CONTEXT][g, q, c, 1]))
        return "".join(rows)
