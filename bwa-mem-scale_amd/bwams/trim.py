"""Read trimming before mapping, restated in plain numpy / Python: rules T1 to T9 above bwams_fastq_trim in include/bwams.h.

A read is a tuple (name: bytes, comment: bytes | None, codes: uint8 array of 0..4, quals: uint8 array of the FASTQ bytes | None).
trim() is the yardstick of csrc/trim.hip: the device's arrays, report and stats equal it entry for entry."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

OVERLAP_MAX_LEN = 1024                                   # BWAMS_TRIM_OVERLAP_MAX_LEN
KEPT, LEN, N, QUAL, MATE = 0, 1, 2, 3, 4                 # bwams_trim_read_t.reason
S_FIXED, S_CUT_FRONT, S_CUT_TAIL, S_OVERLAP, S_ADAPTER, S_MAX_LEN = range(6)      # the steps: bit k of .steps, entry k of .removed
STEP_SKIPPED = 0x40                                      # .steps: the pair was too long for T3
READ_DTYPE = np.dtype([("start", "<i4"), ("len", "<i4"), ("insert", "<i4"), ("reason", "u1"), ("steps", "u1"), ("pad_", "u1", (2,)),
                       ("removed", "<i4", (6,))])        # bwams_trim_read_t
assert READ_DTYPE.itemsize == 40


@dataclass
class Opt:
    """bwams_trim_opt_t with bwams_trim_opt_default's values"""
    trim_front: int = 0
    trim_tail: int = 0
    cut_front: int = 0
    cut_tail: int = 1
    cut_window: int = 4
    cut_quality: int = 20
    overlap: int = 1
    overlap_min: int = 30
    overlap_max_diff: int = 5
    overlap_diff_pct: int = 20
    adapter_min_match: int = 4
    adapter_mismatch_per: int = 8
    max_len: int = 0
    min_len: int = 15
    n_limit: int = 5
    qual_floor: int = 15
    low_qual_pct: int = 40
    adapter1: bytes = b""
    adapter2: bytes = b""


def identity_opt(**kw) -> Opt:
    """every step off and filters that pass every read of at least one base"""
    o = Opt(cut_tail=0, overlap=0, min_len=1, n_limit=2**31 - 1, qual_floor=0, low_qual_pct=100)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def check_opt(o, n_reads: int, paired: bool) -> None:
    """T9: ValueError naming the field"""
    def bad(f):
        raise ValueError(f)
    for f in ("trim_front", "trim_tail", "cut_quality", "overlap_max_diff", "overlap_diff_pct", "max_len", "n_limit", "qual_floor",
              "low_qual_pct"):
        if getattr(o, f) < 0:
            bad(f)
    if not 1 <= o.cut_window <= 64:
        bad("cut_window")
    for f in ("overlap_min", "adapter_min_match", "adapter_mismatch_per", "min_len"):
        if getattr(o, f) < 1:
            bad(f)
    for f in ("adapter1", "adapter2"):
        a = bytes(getattr(o, f))
        if len(a) > 128 or any(c not in b"ACGT" for c in a):
            bad(f)
    if paired and n_reads & 1:
        bad("paired")


def _q(quals) -> np.ndarray:
    q = np.asarray(quals, np.int64) - 33
    q[q < 0] = 0
    return q


def _first_window(q: np.ndarray, w0: int, Q: int) -> int:
    """the smallest s whose window passes, moved on past the bases below Q; -1 when no window passes"""
    n = len(q)
    w = min(w0, n)
    E = np.concatenate([[0], np.cumsum(q)])
    ok = np.nonzero(E[w:n + 1] - E[0:n - w + 1] >= w * Q)[0]
    if len(ok) == 0:
        return -1
    s = int(ok[0])
    while q[s] < Q:
        s += 1
    return s


def find_insert(c1: np.ndarray, c2: np.ndarray, o) -> int:
    """T3: the largest passing insert length, or 0"""
    n1, n2 = len(c1), len(c2)
    a = np.asarray(c1, np.uint8)
    r = np.asarray(c2, np.uint8)[::-1]
    b = np.where(r == 4, 4, 3 - r).astype(np.uint8)
    for I in range(n1 + n2 - o.overlap_min, o.overlap_min - 1, -1):
        lo, hi = max(0, I - n2), min(n1, I)
        ov = hi - lo
        if ov < o.overlap_min:
            continue
        x, y = a[lo:hi], b[lo + n2 - I:hi + n2 - I]
        d = int(np.count_nonzero((x != y) | (x == 4) | (y == 4)))
        if d <= o.overlap_max_diff and 100 * d <= o.overlap_diff_pct * ov:
            return I
    return 0


def _codes(adapter: bytes) -> np.ndarray:
    return np.array([b"ACGT".index(c) for c in bytes(adapter)], np.uint8)


def find_adapter(c: np.ndarray, A: np.ndarray, o) -> int:
    """T4: the smallest p at which the adapter is taken to start, or -1"""
    n, m = len(c), len(A)
    if m == 0:
        return -1
    c = np.asarray(c, np.uint8)
    for p in range(0, n - o.adapter_min_match + 1):
        cmp_ = min(n - p, m)
        x = c[p:p + cmp_]
        d = int(np.count_nonzero((x != A[:cmp_]) | (x == 4)))
        if d * o.adapter_mismatch_per <= cmp_:
            return p
    return -1


def _find_insert_all(c1: np.ndarray, c2: np.ndarray, o) -> int:
    """find_insert with every candidate's d at once (trim() uses it; test_trim.py holds it to find_insert): the positions that pair
    under I are one diagonal of the n1 x n2 table of mismatches, j - i = n2 - I"""
    n1, n2 = len(c1), len(c2)
    if n1 == 0 or n2 == 0 or n1 + n2 - o.overlap_min < o.overlap_min:
        return 0
    a = np.asarray(c1, np.uint8)
    r = np.asarray(c2, np.uint8)[::-1]
    b = np.where(r == 4, 4, 3 - r).astype(np.uint8)
    i, j = np.nonzero((a[:, None] != b[None, :]) | (a == 4)[:, None] | (b == 4)[None, :])
    by_diag = np.bincount(j - i + (n1 - 1), minlength=n1 + n2 - 1)
    I = np.arange(o.overlap_min, n1 + n2 - o.overlap_min + 1)
    d = by_diag[n2 - I + n1 - 1]
    ov = np.minimum(n1, I) - np.maximum(0, I - n2)
    ok = np.nonzero((ov >= o.overlap_min) & (d <= o.overlap_max_diff) & (100 * d <= o.overlap_diff_pct * ov))[0]
    return int(I[ok[-1]]) if len(ok) else 0


def _find_adapter_all(c: np.ndarray, A: np.ndarray, o) -> int:
    """find_adapter with every position's d at once (trim() uses it; test_trim.py holds it to find_adapter)"""
    n, m = len(c), len(A)
    last = n - o.adapter_min_match
    if m == 0 or last < 0:
        return -1
    c = np.asarray(c, np.uint8)
    for p0 in range(0, last + 1, 4096):                  # blocks of positions: the table stays small for a long read
        p = np.arange(p0, min(last, p0 + 4095) + 1)
        at = p[:, None] + np.arange(m)[None, :]
        x = c[np.minimum(at, n - 1)]
        cmp_ = np.minimum(n - p, m)
        d = (((x != A[None, :]) | (x == 4)) & (at < n)).sum(axis=1)
        ok = np.nonzero(d * o.adapter_mismatch_per <= cmp_)[0]
        if len(ok):
            return int(p[ok[0]])
    return -1


class _End:
    def __init__(self, read):
        self.c = np.asarray(read[2], np.uint8)
        self.q = _q(read[3]) if read[3] is not None else None
        self.s, self.e = 0, len(self.c)
        self.removed = [0] * 6
        self.insert = 0
        self.skipped = False

    @property
    def n(self):
        return self.e - self.s

    def cut(self, step, s, e):
        self.removed[step] += self.n - (e - s)
        self.s, self.e = s, e

    def before_overlap(self, o):                         # T1, T2
        n = self.n
        s = min(n, o.trim_front)
        self.cut(S_FIXED, s, max(s, n - o.trim_tail))
        if self.q is None:
            return
        if o.cut_front and self.n > 0:
            k = _first_window(self.q[self.s:self.e], o.cut_window, o.cut_quality)
            self.cut(S_CUT_FRONT, self.s + k, self.e) if k >= 0 else self.cut(S_CUT_FRONT, self.s, self.s)
        if o.cut_tail and self.n > 0:
            k = _first_window(self.q[self.s:self.e][::-1], o.cut_window, o.cut_quality)
            self.cut(S_CUT_TAIL, self.s, self.e - k) if k >= 0 else self.cut(S_CUT_TAIL, self.s, self.s)

    def after_overlap(self, o, adapter):                 # T4 (no insert found), T5
        if not self.insert:
            p = _find_adapter_all(self.c[self.s:self.e], adapter, o)
            if p >= 0:
                self.cut(S_ADAPTER, self.s, self.s + p)
        if o.max_len > 0 and self.n > o.max_len:
            self.cut(S_MAX_LEN, self.s, self.s + o.max_len)

    def reason(self, o):                                 # T6
        c = self.c[self.s:self.e]
        if self.n < o.min_len:
            return LEN
        if int(np.count_nonzero(c == 4)) > o.n_limit:
            return N
        if self.q is not None and 100 * int(np.count_nonzero(self.q[self.s:self.e] < o.qual_floor)) > o.low_qual_pct * self.n:
            return QUAL
        return KEPT


def stats_of(report: np.ndarray, lens, paired: bool) -> dict:
    """T8: every number from the report (and the input lengths)"""
    lens = np.asarray(lens, np.int64)
    kept = report["reason"] == KEPT
    first = report[0::2] if paired else report[:0]
    st = dict(reads_in=len(report), bases_in=int(lens.sum()), reads_out=int(kept.sum()), bases_out=int(report["len"][kept].astype(np.int64).sum()),
              pairs_insert=int((first["insert"] > 0).sum()), pairs_skipped=int(((first["steps"] & STEP_SKIPPED) != 0).sum()),
              step_reads=[int((report["removed"][:, k] > 0).sum()) if len(report) else 0 for k in range(6)],
              step_bases=[int(report["removed"][:, k].astype(np.int64).sum()) if len(report) else 0 for k in range(6)],
              dropped=[int((report["reason"] == r).sum()) for r in (LEN, N, QUAL, MATE)])
    return st


def trim(reads, opt, paired: bool = False):
    """-> (kept reads, report (READ_DTYPE, one entry per input read), stats dict)"""
    check_opt(opt, len(reads), paired)
    ad = [_codes(opt.adapter1), _codes(opt.adapter2)]
    ends = [_End(r) for r in reads]
    report = np.zeros(len(reads), READ_DTYPE)
    reasons = [KEPT] * len(reads)
    for i in range(0, len(reads), 2 if paired else 1):
        unit = ends[i:i + 2] if paired else ends[i:i + 1]
        for e in unit:
            e.before_overlap(opt)
        if paired and opt.overlap:
            a, b = unit
            if a.n > OVERLAP_MAX_LEN or b.n > OVERLAP_MAX_LEN:
                a.skipped = b.skipped = True
            else:
                I = _find_insert_all(a.c[a.s:a.e], b.c[b.s:b.e], opt)
                if I:
                    for e in unit:
                        e.insert = I
                        e.cut(S_OVERLAP, e.s, e.s + min(e.n, I))
        for k, e in enumerate(unit):
            e.after_overlap(opt, ad[k])
        rs = [e.reason(opt) for e in unit]
        if any(rs):
            rs = [r or MATE for r in rs]
        reasons[i:i + len(unit)] = rs
    for i, e in enumerate(ends):
        r = report[i]
        r["start"], r["len"], r["insert"], r["reason"] = e.s, e.n, e.insert, reasons[i]
        r["removed"] = e.removed
        r["steps"] = sum(1 << k for k in range(6) if e.removed[k]) | (STEP_SKIPPED if e.skipped else 0)
    kept = []
    for i, (name, comment, c, q) in enumerate(reads):
        if reasons[i] == KEPT:
            s, e = ends[i].s, ends[i].e
            kept.append((name, comment, np.asarray(c, np.uint8)[s:e].copy(), None if q is None else np.asarray(q, np.uint8)[s:e].copy()))
    return kept, report, stats_of(report, [len(r[2]) for r in reads], paired)


def from_fetch(d: dict) -> list:
    """the reads of capi.Fastq.fetch()"""
    cum = d["cum"]
    return [(d["names"][k], d["comments"][k], d["enc"][cum[k]:cum[k + 1]], None if d["quals"] is None else d["quals"][cum[k]:cum[k + 1]])
            for k in range(d["n"])]


def to_fastq(reads, with_comment: bool = True) -> bytes:
    """bwams_fastq_text: '@name[ comment]\\nSEQ\\n+\\nQUAL\\n' per read, or '>name[ comment]\\nSEQ\\n' without qualities"""
    out = []
    for name, comment, c, q in reads:
        head = bytes(name) + (b" " + bytes(comment) if with_comment and comment else b"")
        seq = bytes(b"ACGTN"[x] for x in c)
        out.append(b">" + head + b"\n" + seq + b"\n" if q is None else b"@" + head + b"\n" + seq + b"\n+\n" + bytes(bytearray(q)) + b"\n")
    return b"".join(out)
