"""Pileup restated in numpy: the yardstick of csrc/pileup.hip and host/pileup_text.cpp.

The rules are numbered in include/bwams.h above bwams_pileup_open; the numbers below are theirs.  Pileup(l_ref, regions, ...)
accumulates records (BAM records with their block_size, back to back, as bwams/bam.py builds them) into 12 counters per region
position; fetch, sites and text return what the C-ABI's return.  After set_quality the adds also keep rule 11's sums, 12 per position,
and fetch_quality, calls and vcf restate rules 10 to 13 (csrc/pileup.hip's quality sinks and call kernel, host/pileup_vcf.cpp) in integer
arithmetic alone.  After set_indels the adds also keep rule 14's events and rule 15's span sums, and fetch_span, indel_alleles,
indel_calls, indel_vcf and vcf_all restate rules 14 to 17 (csrc/pileup_indel.hip, host/pileup_indel_vcf.cpp):
 14. Every I or D op of a counted record that a reference-consuming op precedes is an event at the anchor, the position before the op;
     dropped when the anchor has no slot.  (type, len, seq): 0 DEL, 1 INS, 2 OTHER; seq packs an insertion's bases 2 bits each, base j
     at bits 2j.  OTHER, with len 0 and seq 0: longer than max_len, an inserted base that is not A C G T, or a deletion whose last
     position is not in the anchor's region.  qe = clamp(min(MAPQ, indel_q), 4, 60).
 15. A counted record spans slot s when s and s + 1 lie in one maximal run of M/=/X ops; SPAN_N, SPAN_Q, SPAN_HOM, SPAN_HET get 1, qe,
     T_HOM[qe], T_HET[qe], modulo 2^32.
 16. At a slot with reference base < 4 the events group by (type, len, seq); ALT is the type-0 or type-1 group of largest n, the first
     in that order on a tie; cost(RR) = SPAN_HOM + MIS_ALT, cost(RA) = SPAN_HET + HET_ALT, cost(AA) = SPAN_MIS + HOM_ALT with
     MIS = 100 Q + 477 n; pl, genotype, qual and gq as rule 13; depth = SPAN_N + n_ALT + n_other; a call when the genotype is not RR,
     qual >= min_qual and depth >= min_depth.  No realignment, no model of repeats, strands or mate overlap; the alleles are as the
     CIGARs give them unless rule 18 is on.
 17. INDEL_DTYPE and INDEL_ALLELE_DTYPE records; the VCF rows with INFO DP=depth;INDEL, and vcf_all's merge, the SNV first at a slot.
 18. Left-alignment (set_indel_leftalign; the reference before the records).  A DEL or INS event (rule 14's type, taken first) of
     length L >= 1 at anchor a in region [beg, end): X is the reference up to a, then the reference (DEL) or the inserted bases (INS);
     k is the largest shift with a - j - 1 >= beg, X[a - j] == X[a + L - j] and neither an N, for every j < k.  The event is stored at
     a - k, an insertion's sequence as X[a - k + 1 .. a - k + L].  When the op directly before the event's op is M, = or X, the record
     does not span the slots of [a - k, a) that lie in that run.  Nothing else moves: not the DEL and INS channels, not an earlier run.
"""
from __future__ import annotations

import struct

import numpy as np

from bwams import bam

DEFAULT_EXCLUDE = 0x704
CHANNELS = ("A+", "C+", "G+", "T+", "A-", "C-", "G-", "T-", "N", "DEL", "INS")          # the live ones; channel 11 stays 0
N, DEL, INS = 8, 9, 10
KINDS = ("A", "C", "G", "T", "DEL", "INS")                                              # rule 8's bits 0..5
SITE_DTYPE = np.dtype([("region", "<i4"), ("pos", "<i4"), ("ref", "<i4"), ("kinds", "<u4"), ("depth", "<u4"), ("c", "<u4", (12,))])
TEXT_HEADER = "chrom\tpos\tref\tdepth\t" + "\t".join(CHANNELS) + "\talt\n"
_CHANNEL_OF_CODE = np.full(16, N, np.int64)                                             # rule 4: every code but 1 2 4 8 is N
_CHANNEL_OF_CODE[[1, 2, 4, 8]] = [0, 1, 2, 3]
_REF_OPS, _QUERY_OPS = (0, 2, 3, 7, 8), (0, 1, 4, 7, 8)
# Rule 12: the cost, in hundredths of a phred, of a base of effective quality GL_MIN_Q + k under a homozygous and under a heterozygous
# genotype that holds it (csrc/common.h has the same numbers; tests/test_pileup_calls.py recomputes them); a mismatch costs 100 q + GL_MIS.
GL_MIN_Q, GL_MAX_Q, GL_MIS = 4, 60, 477
T_HOM = (220, 165, 126, 97, 75, 58, 46, 36, 28, 22, 18, 14, 11, 9, 7, 6, 4, 3, 3, 2, 2, 1, 1, 1, 1, 1) + (0,) * 31
T_HET = (435, 404, 381, 363, 350, 339, 331, 325, 320, 316, 313, 310, 308, 307, 306, 305, 304, 303, 303, 302, 302, 302, 302, 302) + (301,) * 33
Q, HOM, HET = 0, 4, 8                                                                   # rule 11: the sums of base b at these + b
GENOTYPES = tuple((a1, a2) for a2 in range(4) for a1 in range(a2 + 1))                  # rule 13: index a2 (a2 + 1) / 2 + a1
CALL_DTYPE = np.dtype([("region", "<i4"), ("pos", "<i4"), ("ref", "<i4"), ("a1", "<i4"), ("a2", "<i4"), ("qual", "<i4"), ("gq", "<i4"),
                       ("depth", "<u4"), ("n", "<u4", (4,)), ("pl", "<i4", (10,))])
VCF_FIXED = ('##INFO=<ID=DP,Number=1,Type=Integer,Description="Bases counted">\n'
             '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
             '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Bases counted per allele">\n'
             '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Bases counted">\n'
             '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality">\n'
             '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Genotype costs in phred, the least at 0">\n'
             "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t")
EV_DEL, EV_INS, EV_OTHER = 0, 1, 2                                                      # rule 14's types
SPAN_N, SPAN_Q, SPAN_HOM, SPAN_HET = 0, 1, 2, 3                                         # rule 15's sums
INDEL_MAX = 32
INDEL_DTYPE = np.dtype([("region", "<i4"), ("pos", "<i4"), ("ref", "<i4"), ("type", "<i4"), ("len", "<i4"), ("reserved", "<i4"), ("seq", "<u8"),
                        ("gt", "<i4"), ("qual", "<i4"), ("gq", "<i4"), ("depth", "<u4"), ("n_ref", "<u4"), ("n_alt", "<u4"), ("n_other", "<u4"),
                        ("pl", "<i4", (3,)), ("del_ref", "u1", (INDEL_MAX,))])          # bwams_pileup_indel_t
INDEL_ALLELE_DTYPE = np.dtype([("region", "<i4"), ("pos", "<i4"), ("type", "<i4"), ("len", "<i4"), ("seq", "<u8"), ("n", "<u8"), ("q", "<u8"),
                               ("hom", "<u8"), ("het", "<u8")])                          # bwams_pileup_indel_allele_t
assert INDEL_DTYPE.itemsize == 104 and INDEL_ALLELE_DTYPE.itemsize == 56
VCF_INDEL_LINE = '##INFO=<ID=INDEL,Number=0,Type=Flag,Description="An insertion or deletion, as the CIGARs give it">\n'


class PileupRefusal(ValueError):
    """Rule 3 (BWAMS_ERR_ARG); .record is the record's index in the call, .why "op", "length" or "bounds"."""

    def __init__(self, record: int, why: str):
        super().__init__(f"record {record}: {why}")
        self.record, self.why = record, why


def fields(rec: bytes):
    """(refID, POS, MAPQ, FLAG, [(length, op)], l_seq, codes uint8[l_seq], qual uint8[l_seq]) of one record (block_size included)."""
    refid, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 4)
    at = 36 + l_name
    ops = struct.unpack_from("<%dI" % n_cig, rec, at)
    at += 4 * n_cig
    n = min(max(l_seq, 0), max(len(rec) - at, 0) * 2 // 3)                        # a record cut short: rule 3 refuses it when it counts
    packed = np.frombuffer(rec, np.uint8, (n + 1) // 2, at)
    codes = np.stack([packed >> 4, packed & 15], 1).reshape(-1)[:n]
    qual = np.frombuffer(rec, np.uint8, n, at + (n + 1) // 2)
    return refid, pos, mapq, flag, [(c >> 4, c & 15) for c in ops], l_seq, codes, qual


class Pileup:
    def __init__(self, l_ref, regions=(), exclude: int = DEFAULT_EXCLUDE, min_mapq: int = 0, min_baseq: int = 13, min_alt: int = 2,
                 min_permille: int = 200):
        self.l_ref = [int(x) for x in l_ref]
        regions = [tuple(int(v) for v in r) for r in regions] or [(r, 0, n) for r, n in enumerate(self.l_ref) if n > 0]
        for k, (r, b, e) in enumerate(regions):                                          # rule 1
            assert 0 <= r < len(self.l_ref) and 0 <= b < e <= self.l_ref[r], (k, r, b, e)
            assert k == 0 or (regions[k - 1][0], regions[k - 1][2]) <= (r, b), "sorted, no overlap"
        self.regions = regions
        self.off = np.concatenate([[0], np.cumsum([e - b for _, b, e in regions])]).astype(np.int64)
        self.n_slots = int(self.off[-1])
        self.slot = [np.full(n, -1, np.int64) for n in self.l_ref]                       # position -> slot, -1 outside every region
        for k, (r, b, e) in enumerate(regions):
            self.slot[r][b:e] = np.arange(self.off[k], self.off[k + 1])
        self.exclude, self.min_mapq, self.min_baseq, self.min_alt, self.min_permille = exclude, min_mapq, min_baseq, min_alt, min_permille
        self.ref = np.full(self.n_slots, 4, np.uint8)                                    # rule 7
        self.q = None                                                                    # rule 11's plane: none before set_quality
        self.span = None                                                                 # rule 15's sums: none before set_indels
        self.leftalign = False                                                           # rule 18: off before set_indel_leftalign
        self.ref_set = [False] * len(regions)                                            # ... which wants every region's bases before an add
        self.reset()

    def reset(self):                                                                     # rule 6
        self.dirty = False                                                               # an add since the open or the last reset
        self.c = np.zeros((self.n_slots, 12), np.int64)
        if self.q is not None:
            self.q = np.zeros((self.n_slots, 12), np.int64)
        if self.span is not None:
            self.span = np.zeros((self.n_slots, 4), np.int64)
            self.events = []                                                             # (slot, type, len, seq, qe, from an I op)

    def set_indels(self, min_qual: int = 20, min_depth: int = 1, indel_q: int = 40, max_len: int = INDEL_MAX):
        """the indel store, empty; only while the counters are zero (BWAMS_ERR_ARG otherwise)"""
        assert min_qual >= 0 and min_depth >= 1 and 0 <= indel_q <= 93 and 1 <= max_len <= INDEL_MAX and not self.c.any()
        assert self.n_slots < 2 ** 32
        self.indel_min_qual, self.indel_min_depth, self.indel_q, self.max_len = min_qual, min_depth, indel_q, max_len
        self.span = np.zeros((self.n_slots, 4), np.int64)
        self.events = []
        self.leftalign = False                                                           # the call replaces the store's options

    def set_indel_leftalign(self, on: bool = True):
        """rule 18 for the adds that follow; only on a handle with the store and while the counters are zero (BWAMS_ERR_ARG otherwise)"""
        assert self.span is not None and not self.dirty and on in (0, 1)
        self.leftalign = bool(on)

    def _shift(self, s: int, beg_slot: int, is_ins: bool, n: int, seq: int):
        """rule 18's k and the sequence at the new anchor, one base at a time; s: the anchor's slot, beg_slot: its region's first.
        Inside a region the slots are the positions, so X is indexed by slot."""
        def X(t):
            return int(self.ref[t]) if t <= s or not is_ins else seq >> (2 * (t - s - 1)) & 3
        k = 0
        while s - k - 1 >= beg_slot and X(s - k) != 4 and X(s + n - k) != 4 and X(s - k) == X(s + n - k):
            k += 1
        if is_ins:
            seq = sum(X(s - k + 1 + i) << (2 * i) for i in range(n))
        return k, seq

    def _indels_of(self, refid, pos, mapq, cigar, codes):
        """rules 14 and 15 for one counted record, and rule 18 on a left-aligning handle"""
        qe = min(max(min(mapq, self.indel_q), GL_MIN_Q), GL_MAX_Q)
        add = np.array([1, qe, T_HOM[qe - GL_MIN_Q], T_HET[qe - GL_MIN_Q]], np.int64)
        slot, l_ref = self.slot[refid], self.l_ref[refid]
        x, q, seen, run = pos, 0, False, None
        runs = []
        for n, op in cigar:
            if op in (1, 2) and seen and 0 <= x - 1 < l_ref and slot[x - 1] >= 0:
                s = int(slot[x - 1])
                k = int(np.searchsorted(self.off, s, "right")) - 1                        # the anchor's region
                kind, seq = (EV_INS, 0) if op == 1 else (EV_DEL, 0)
                if n > self.max_len:
                    kind = EV_OTHER
                elif op == 2:
                    if x + n - 1 >= self.regions[k][2]:
                        kind = EV_OTHER
                else:
                    for j, code in enumerate(codes[q:q + n]):
                        if _CHANNEL_OF_CODE[code] > 3:
                            kind = EV_OTHER
                            break
                        seq |= int(_CHANNEL_OF_CODE[code]) << (2 * j)
                if self.leftalign and kind != EV_OTHER and n > 0:                        # rule 18
                    shift, seq = self._shift(s, int(self.off[k]), op == 1, n, seq)
                    if run is not None:                                                  # the op before is M, = or X: its run ends at the anchor
                        gone = max(min(shift, x - 1 - run[0]), 0)                        # [max(a - k, the run's first position), a)
                        self.span[s - gone:s] -= add
                    s -= shift
                self.events.append((s, kind, 0, 0, qe, op == 1) if kind == EV_OTHER else (s, kind, n, seq, qe, op == 1))
            if op in (0, 7, 8):
                run = [x, x + n] if run is None else [run[0], x + n]
            elif run is not None:
                runs.append(run)
                run = None
            if op in _REF_OPS:
                x += n
                seen = True
            if op in _QUERY_OPS:
                q += n
        if run is not None:
            runs.append(run)
        for a, b in runs:                                                                # s and s + 1 in the run: s in [a, b - 1)
            lo, hi = max(a, 0), min(b - 1, l_ref)
            if lo < hi:
                s = slot[lo:hi]
                self.span[s[s >= 0]] += add

    def set_quality(self, min_qual: int = 20, min_depth: int = 1, no_qual_q: int = 30):
        """the quality plane, zeroed; only while the counters are zero (BWAMS_ERR_ARG otherwise)"""
        assert min_qual >= 0 and min_depth >= 1 and 0 <= no_qual_q <= 93 and not self.c.any()
        self.min_qual, self.min_depth, self.no_qual_q = min_qual, min_depth, no_qual_q
        self.q = np.zeros((self.n_slots, 12), np.int64)

    def counts(self, refid, mapq, flag, cigar, l_seq) -> bool:                           # rule 2
        return (not flag & self.exclude and mapq >= self.min_mapq and 0 <= refid < len(self.l_ref) and len(cigar) > 0 and l_seq > 0)

    def _put(self, refid, pos, channel, qe=None):
        """+1 at each (position, channel) whose position lies in a region (rule 4: the others are dropped one by one); with qe, rule
        10's effective quality per position, rule 11's three sums of every base in one of the eight base channels too"""
        pos, channel = np.asarray(pos, np.int64), np.asarray(channel, np.int64)
        ok = (pos >= 0) & (pos < self.l_ref[refid])
        s = self.slot[refid][pos[ok]]
        np.add.at(self.c, (s[s >= 0], channel[ok][s >= 0]), 1)
        if qe is not None:
            s, channel, qe = s[s >= 0], channel[ok][s >= 0], np.asarray(qe, np.int64)[ok][s >= 0]
            s, b, qe = s[channel < 8], channel[channel < 8] & 3, qe[channel < 8]
            np.add.at(self.q, (s, Q + b), qe)
            np.add.at(self.q, (s, HOM + b), np.asarray(T_HOM, np.int64)[qe - GL_MIN_Q])
            np.add.at(self.q, (s, HET + b), np.asarray(T_HET, np.int64)[qe - GL_MIN_Q])

    def add(self, records: bytes) -> int:
        """Every record of `records`; -> the number that counted.  Check first, then add (rule 3)."""
        assert not self.leftalign or all(self.ref_set), "rule 18: every region's reference before the records (BWAMS_ERR_ARG)"
        recs = [fields(r) for r in bam.split_records(records)]
        for k, (refid, _, mapq, flag, cigar, l_seq, codes, _) in enumerate(recs):
            if any(op > 8 for _, op in cigar):
                raise PileupRefusal(k, "op")
            if self.counts(refid, mapq, flag, cigar, l_seq):
                if sum(n for n, op in cigar if op in _QUERY_OPS) != l_seq:
                    raise PileupRefusal(k, "length")
                if len(codes) != l_seq:                                                  # SEQ or QUAL ends behind the record
                    raise PileupRefusal(k, "bounds")
        n_counted = 0
        self.dirty = self.dirty or len(recs) > 0
        for refid, pos, mapq, flag, cigar, l_seq, codes, qual in recs:
            if not self.counts(refid, mapq, flag, cigar, l_seq):
                continue
            n_counted += 1
            strand = 4 if flag & 0x10 else 0
            good = np.ones(l_seq, bool) if qual[0] == 0xFF else qual >= self.min_baseq   # rule 4: no qualities pass every min_baseq
            qe = None
            if self.q is not None:                                                       # rule 10
                raw = np.full(l_seq, self.no_qual_q, np.int64) if qual[0] == 0xFF else qual.astype(np.int64)
                qe = np.clip(np.minimum(raw, mapq), GL_MIN_Q, GL_MAX_Q)
            x, q, seen_ref = pos, 0, False
            for n, op in cigar:
                if op in (0, 7, 8):
                    ch = _CHANNEL_OF_CODE[codes[q:q + n]]
                    ch = np.where(ch < 4, ch + strand, ch)
                    g = good[q:q + n]
                    self._put(refid, np.arange(x, x + n)[g], ch[g], None if qe is None else qe[q:q + n][g])
                elif op == 2:
                    lo, hi = max(x, 0), min(x + n, self.l_ref[refid])
                    if lo < hi:
                        self._put(refid, np.arange(lo, hi), np.full(hi - lo, DEL))
                elif op == 1 and seen_ref:                                               # one per I op, at the position before it
                    self._put(refid, [x - 1], [INS])
                if op in _REF_OPS:
                    x += n
                    seen_ref = True
                if op in _QUERY_OPS:
                    q += n
            if self.span is not None:
                self._indels_of(refid, pos, mapq, cigar, codes)
        return n_counted

    def set_ref(self, region: int, codes):                                               # rule 7
        r, b, e = self.regions[region]
        codes = np.asarray(codes, np.uint8)
        assert len(codes) == e - b and (codes <= 4).all()
        assert not (self.leftalign and self.dirty), "rule 18: the events held were aligned against the bases in place (BWAMS_ERR_ARG)"
        self.ref[self.off[region]:self.off[region + 1]] = codes
        self.ref_set[region] = True

    def set_ref_genome(self, genome_by_ref):
        """every region's bases from one code array per reference (what _set_ref_index gathers)"""
        for k, (r, b, e) in enumerate(self.regions):
            self.set_ref(k, np.minimum(np.asarray(genome_by_ref[r][b:e], np.uint8), 4))

    def fetch(self, region: int, beg: int | None = None, end: int | None = None) -> np.ndarray:
        r, b, e = self.regions[region]
        beg, end = b if beg is None else beg, e if end is None else end
        assert b <= beg <= end <= e
        return self.c[self.off[region] + beg - b:self.off[region] + end - b].astype(np.uint32)

    def sites(self, min_alt: int | None = None, min_permille: int | None = None) -> np.ndarray:      # rule 8
        min_alt = self.min_alt if min_alt is None else min_alt
        min_permille = self.min_permille if min_permille is None else min_permille
        c = self.c
        depth = c[:, :8].sum(1) + c[:, DEL]
        allele = np.stack([c[:, 0] + c[:, 4], c[:, 1] + c[:, 5], c[:, 2] + c[:, 6], c[:, 3] + c[:, 7], c[:, DEL], c[:, INS]], 1)
        cand = (allele >= min_alt) & (allele * 1000 >= min_permille * depth[:, None]) & (self.ref < 4)[:, None]
        cand[:, :4] &= np.arange(4)[None, :] != self.ref[:, None]
        kinds = (cand << np.arange(6)).sum(1)
        at = np.flatnonzero(kinds)
        out = np.zeros(len(at), SITE_DTYPE)
        region = np.searchsorted(self.off, at, "right") - 1
        out["region"] = region
        out["pos"] = at - self.off[region] + np.array([b for _, b, _ in self.regions], np.int64)[region]
        out["ref"], out["kinds"], out["depth"], out["c"] = self.ref[at], kinds[at], depth[at], c[at]
        return out

    def text(self, names, min_alt: int | None = None, min_permille: int | None = None) -> str:       # rule 9
        names = [n.decode() if isinstance(n, bytes) else n for n in names]
        rows = [TEXT_HEADER]
        for s in self.sites(min_alt, min_permille):
            alts = ",".join(k for bit, k in enumerate(KINDS) if int(s["kinds"]) >> bit & 1)
            rows.append("%s\t%d\t%s\t%d\t%s\t%s\n" % (names[self.regions[int(s["region"])][0]], int(s["pos"]) + 1, "ACGTN"[int(s["ref"])],
                                                     int(s["depth"]), "\t".join(str(int(v)) for v in s["c"][:11]), alts))
        return "".join(rows)

    def fetch_quality(self, region: int, beg: int | None = None, end: int | None = None) -> np.ndarray:      # rule 11
        assert self.q is not None
        r, b, e = self.regions[region]
        beg, end = b if beg is None else beg, e if end is None else end
        assert b <= beg <= end <= e
        return self.q[self.off[region] + beg - b:self.off[region] + end - b].astype(np.uint32)

    def genotypes(self) -> np.ndarray:
        """rule 13 at every slot, CALL_DTYPE with region -1 where it does not apply: from the uint32 the device holds (the planes
        modulo 2^32), in Python integers"""
        assert self.q is not None
        out = np.zeros(self.n_slots, CALL_DTYPE)
        out["region"] = -1
        c, q = self.c & 0xFFFFFFFF, self.q & 0xFFFFFFFF
        region = np.searchsorted(self.off, np.arange(self.n_slots), "right") - 1
        for s in np.flatnonzero((self.ref < 4) & (c[:, :8].sum(1) > 0)):
            n = [int(c[s, b]) + int(c[s, b + 4]) for b in range(4)]
            mis = [100 * int(q[s, Q + b]) + GL_MIS * n[b] for b in range(4)]
            cost = [sum(mis[b] if b not in (a1, a2) else int(q[s, (HOM if a1 == a2 else HET) + b]) for b in range(4)) for a1, a2 in GENOTYPES]
            best = cost.index(min(cost))                                                 # ties: the lowest g
            pl = [min((x - cost[best] + 50) // 100, 2 ** 31 - 1) for x in cost]
            r = int(self.ref[s])
            k = int(region[s])
            out[s] = (k, int(s - self.off[k]) + self.regions[k][1], r, GENOTYPES[best][0], GENOTYPES[best][1], pl[r * (r + 1) // 2 + r],
                      min(99, min(x for g, x in enumerate(pl) if g != best)), sum(n) & 0xFFFFFFFF, [x & 0xFFFFFFFF for x in n], pl)
        return out

    def calls(self, min_qual: int | None = None, min_depth: int | None = None) -> np.ndarray:               # rule 13
        min_qual = self.min_qual if min_qual is None else min_qual
        min_depth = self.min_depth if min_depth is None else min_depth
        g = self.genotypes()
        depth = (self.c & 0xFFFFFFFF)[:, :8].sum(1)                                       # untruncated, as the device compares it
        return g[(g["region"] >= 0) & (depth >= min_depth) & ((g["a1"] != g["ref"]) | (g["a2"] != g["ref"])) & (g["qual"] >= min_qual)]

    def vcf(self, names, sample: str, min_qual: int | None = None, min_depth: int | None = None) -> str:
        names = [n.decode() if isinstance(n, bytes) else n for n in names]
        rows = ["##fileformat=VCFv4.2\n##source=bwams\n"]
        rows += ["##contig=<ID=%s,length=%d>\n" % (n, l) for n, l in zip(names, self.l_ref)]
        rows.append(VCF_FIXED + sample + "\n")
        for x in self.calls(min_qual, min_depth):
            r, a1, a2 = int(x["ref"]), int(x["a1"]), int(x["a2"])
            alleles = [r] + [a for a in dict.fromkeys((a1, a2)) if a != r]               # REF, then the other alleles in base order
            gt = sorted((alleles.index(a1), alleles.index(a2)))
            pl = [int(x["pl"][max(alleles[i], alleles[j]) * (max(alleles[i], alleles[j]) + 1) // 2 + min(alleles[i], alleles[j])])
                  for j in range(len(alleles)) for i in range(j + 1)]
            rows.append("%s\t%d\t.\t%s\t%s\t%d\t.\tDP=%d\tGT:AD:DP:GQ:PL\t%d/%d:%s:%d:%d:%s\n" % (
                names[self.regions[int(x["region"])][0]], int(x["pos"]) + 1, "ACGT"[r], ",".join("ACGT"[a] for a in alleles[1:]), int(x["qual"]),
                int(x["depth"]), gt[0], gt[1], ",".join(str(int(x["n"][a])) for a in alleles), int(x["depth"]), int(x["gq"]),
                ",".join(map(str, pl))))
        return "".join(rows)

    def fetch_span(self, region: int, beg: int | None = None, end: int | None = None) -> np.ndarray:           # rule 15
        assert self.span is not None
        r, b, e = self.regions[region]
        beg, end = b if beg is None else beg, e if end is None else end
        assert b <= beg <= end <= e
        return self.span[self.off[region] + beg - b:self.off[region] + end - b].astype(np.uint32)

    def _place(self, s: int):
        k = int(np.searchsorted(self.off, s, "right")) - 1
        return k, int(s - self.off[k]) + self.regions[k][1]

    def _groups(self):
        """{slot: [((type, len, seq), [n, Q, HOM, HET]), ...] in rule 16's order}, the slots ascending"""
        assert self.span is not None
        g = {}
        for s, kind, n, seq, qe, _ in self.events:
            v = g.setdefault((s, kind, n, seq), [0, 0, 0, 0])
            v[0] += 1; v[1] += qe; v[2] += T_HOM[qe - GL_MIN_Q]; v[3] += T_HET[qe - GL_MIN_Q]
        by_slot = {}
        for key in sorted(g):
            by_slot.setdefault(key[0], []).append((key[1:], g[key]))
        return by_slot

    def indel_alleles(self) -> np.ndarray:                                               # rule 17: every group, OTHER included
        rows = [(*self._place(s), kind, n, seq, *v) for s, groups in self._groups().items() for (kind, n, seq), v in groups]
        out = np.zeros(len(rows), INDEL_ALLELE_DTYPE)
        for i, row in enumerate(rows):
            out[i] = row
        return out

    def indel_genotypes(self):
        """rule 16 at every slot that has an ALT: [(INDEL_DTYPE record, depth untruncated, tie)], tie: another type-0 or type-1 group
        has the ALT's n"""
        out = []
        span = self.span & 0xFFFFFFFF
        for s, groups in self._groups().items():
            r = int(self.ref[s])
            cand = [(key, v) for key, v in groups if key[0] != EV_OTHER]
            if r > 3 or not cand:
                continue
            n_alt = max(v[0] for _, v in cand)
            (kind, n, seq), alt = next((key, v) for key, v in cand if v[0] == n_alt)      # a tie: the first in the order
            total = sum(v[0] for _, v in groups)
            sp = [int(x) for x in span[s]]
            cost = [sp[SPAN_HOM] + 100 * alt[1] + GL_MIS * alt[0], sp[SPAN_HET] + alt[3], 100 * sp[SPAN_Q] + GL_MIS * sp[SPAN_N] + alt[2]]
            best = cost.index(min(cost))
            pl = [min((x - cost[best] + 50) // 100, 2 ** 31 - 1) for x in cost]
            k, pos = self._place(s)
            rec = np.zeros(1, INDEL_DTYPE)[0]
            depth = sp[SPAN_N] + total
            del_ref = np.zeros(INDEL_MAX, np.uint8)
            if kind == EV_DEL:
                del_ref[:n] = self.ref[s + 1:s + 1 + n]
            rec["region"], rec["pos"], rec["ref"], rec["type"], rec["len"], rec["seq"], rec["gt"] = k, pos, r, kind, n, seq, best
            rec["qual"], rec["gq"], rec["depth"] = pl[0], min(99, min(x for g, x in enumerate(pl) if g != best)), depth & 0xFFFFFFFF
            rec["n_ref"], rec["n_alt"], rec["n_other"] = sp[SPAN_N], n_alt & 0xFFFFFFFF, (total - n_alt) & 0xFFFFFFFF
            rec["pl"], rec["del_ref"] = pl, del_ref
            out.append((rec, depth, sum(v[0] == n_alt for _, v in cand) > 1))
        return out

    def indel_calls(self, min_qual: int | None = None, min_depth: int | None = None) -> np.ndarray:         # rule 16
        min_qual = self.indel_min_qual if min_qual is None else min_qual
        min_depth = self.indel_min_depth if min_depth is None else min_depth
        rows = [rec for rec, depth, _ in self.indel_genotypes() if rec["gt"] != 0 and rec["qual"] >= min_qual and depth >= min_depth]
        return np.array(rows, INDEL_DTYPE) if rows else np.zeros(0, INDEL_DTYPE)

    def _vcf_head(self, names, sample: str, indel: bool):
        fixed = VCF_FIXED.split("\n", 1)
        return (["##fileformat=VCFv4.2\n##source=bwams\n"] + ["##contig=<ID=%s,length=%d>\n" % (n, l) for n, l in zip(names, self.l_ref)] +
                [fixed[0] + "\n" + (VCF_INDEL_LINE if indel else "") + fixed[1] + sample + "\n"])

    def _indel_row(self, names, x) -> str:                                               # rule 17
        r, n = "ACGT"[int(x["ref"])], int(x["len"])
        if int(x["type"]) == EV_DEL:
            ref, alt = r + "".join("ACGTN"[c] for c in x["del_ref"][:n]), r
        else:
            ref, alt = r, r + "".join("ACGT"[int(x["seq"]) >> (2 * j) & 3] for j in range(n))
        return "%s\t%d\t.\t%s\t%s\t%d\t.\tDP=%d;INDEL\tGT:AD:DP:GQ:PL\t%s:%d,%d:%d:%d:%d,%d,%d\n" % (
            names[self.regions[int(x["region"])][0]], int(x["pos"]) + 1, ref, alt, int(x["qual"]), int(x["depth"]),
            "0/1" if int(x["gt"]) == 1 else "1/1", int(x["n_ref"]), int(x["n_alt"]), int(x["depth"]), int(x["gq"]), *map(int, x["pl"]))

    def indel_vcf(self, names, sample: str, min_qual: int | None = None, min_depth: int | None = None) -> str:
        names = [n.decode() if isinstance(n, bytes) else n for n in names]
        return "".join(self._vcf_head(names, sample, True) + [self._indel_row(names, x) for x in self.indel_calls(min_qual, min_depth)])

    def vcf_all(self, names, sample: str, min_qual: int | None = None, min_depth: int | None = None, indel_min_qual: int | None = None,
                indel_min_depth: int | None = None) -> str:
        """the SNV rows of vcf and the indel rows of indel_vcf under the header with the INDEL line, by (region, pos), the SNV first"""
        assert self.q is not None and self.span is not None
        names = [n.decode() if isinstance(n, bytes) else n for n in names]
        snv_rows = self.vcf(names, sample, min_qual, min_depth).splitlines(True)[len(names) + 2 + VCF_FIXED.count("\n") + 1:]
        rows = [((int(x["region"]), int(x["pos"]), 0), row) for x, row in zip(self.calls(min_qual, min_depth), snv_rows)]
        rows += [((int(x["region"]), int(x["pos"]), 1), self._indel_row(names, x)) for x in self.indel_calls(indel_min_qual, indel_min_depth)]
        return "".join(self._vcf_head(names, sample, True) + [row for _, row in sorted(rows)])
