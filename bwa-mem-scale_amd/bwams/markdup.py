"""Duplicate marking restated in Python: the yardstick of csrc/markdup.hip and of the sorter's BWAMS_SORT_MARKDUP.

These are Picard MarkDuplicates' rules for query-grouped input: default SUM_OF_BASE_QUALITIES scoring, one library, no optical
duplicate detection, no barcodes.  Neither Picard nor samtools is a dependency, so the rules below are the specification:

1. Template: a maximal run of consecutive records with byte-equal read names, in the batch's unsorted order.  This is the order
   bwams_bam_run produces, and the order an uploaded BAM is given in.  A template never spans two batches or two sorter puts.
2. Primary: FLAG has neither 0x100 nor 0x800.  A primary's segment is "only" when 0x1 is clear.  When 0x1 is set, it is "first"
   for 0x40 and "last" for 0x80.  A template is refused with BWAMS_ERR_UNSUPPORTED in any of these cases, and bwams_last_error
   names the first record concerned:
   - two primaries of one segment (for example, two adjacent single-end reads that share a name);
   - a paired primary with neither or both of 0x40/0x80;
   - paired and unpaired primaries mixed.
3. Unclipped 5' coordinate of a mapped primary (0x4 clear), 0-based:
   - forward: POS - (the S and H lengths before the first other op);
   - reverse (0x10): POS + rlen - 1 + (the S and H lengths after the last other op), where rlen is the sum of the M/D/N/=/X lengths,
     taken as 1 when it is 0.
   A coordinate outside [-2^31, 2^31) is refused as in rule 2.
4. Score of a mapped primary: the sum of its QUAL values that are >= 15, capped at 16383 (Picard's Short.MAX_VALUE / 2).  It is
   0 when QUAL is absent (0xFF).  A pair's score is the sum of its two ends' scores.
5. Ends:
   - Pair: a template whose two primaries ("first" and "last") are both mapped.  End 1 is the end with the smaller
     (refID, coordinate); on a tie it is the earlier record.  The pair key is (ref1, c1, strand1, ref2, c2, strand2), so FR and RF at
     the same places are different keys.
   - Fragment: any other template with exactly one mapped primary.  The fragment key is (ref, c, strand).
   - Each end of a pair is also a paired fragment under its own fragment key, for rule 6 only.
6. Decision.  The tie-break "earlier" below means input order: the batch's record order, and across sorter puts, seq first.
   - Pairs with equal keys: the pair with the highest score is kept.  Ties go to the earlier template.  Every other pair is a
     duplicate.
   - Fragments with equal keys: if the group holds any paired fragment, every unpaired fragment in it is a duplicate.  Otherwise the
     highest score is kept, ties go to the earlier template, and the rest are duplicates.
7. Marking: every record of a duplicate template gets FLAG 0x400.  That includes its primaries, its secondary and supplementary
   records, and the unmapped mate of a duplicate fragment.  This is what Picard does on query-grouped input.  Every other record has
   0x400 cleared.  Templates with no mapped primary are never duplicates.  Nothing but that one FLAG bit changes, so sizes, bins and
   the BAI stay the same.
8. Counts: templates (all templates); unpaired_examined / unpaired_duplicates (fragments, and the fragments marked); pairs_examined /
   pair_duplicates (pairs, not reads, and the pairs marked); records_marked (records that end up with 0x400 set).  Picard's
   PERCENT_DUPLICATION is (unpaired_duplicates + 2 pair_duplicates) / (unpaired_examined + 2 pairs_examined).

Where rule 2 says "the first record concerned": the templates are walked record by record in order, and a template's fault is the
record at which the walk meets it (the second primary of a segment, a paired primary without exactly one of 0x40 / 0x80, the first
primary whose 0x1 differs from the template's first primary's, a mapped primary whose coordinate is out of range or whose refID is
-1); the first record concerned is the smallest such record over the batch.

templates(records) -> [(first, end)] (rule 1); ends(records) -> (n_templates, ends, rec_tmpl), refusing with MarkdupRefusal;
decide(ends, n_templates) -> (dup per template, counts); mark(runs) -> (marked records per run, counts), runs in seq order.
An end is a dict with the fields of bwams_dup_end_t: tmpl, ref1, pos1, ref2 (-1 for a fragment), pos2, score, strands.
"""
from __future__ import annotations

import itertools
import struct

from .bam import split_records

QUAL_MIN, SCORE_CAP = 15, 16383
REASONS = ("two primaries of one segment", "a paired primary with neither or both of 0x40 / 0x80",
           "paired and unpaired primaries mixed", "a mapped primary's unclipped 5' coordinate outside [-2^31, 2^31) or its refID -1")


class MarkdupRefusal(ValueError):
    """A batch the rules refuse (BWAMS_ERR_UNSUPPORTED); .record is the first record concerned, .reason the index into REASONS."""

    def __init__(self, record: int, reason: int):
        super().__init__(f"record {record}: {REASONS[reason]}")
        self.record = record
        self.reason = reason


def _records(records) -> list[bytes]:
    return split_records(records) if isinstance(records, (bytes, bytearray)) else list(records)


def _name(rec: bytes) -> bytes:
    return rec[36:36 + rec[12]]


def _flag(rec: bytes) -> int:
    return struct.unpack_from("<H", rec, 18)[0]


def templates(records) -> list[tuple[int, int]]:
    """Rule 1: the templates of records (a list of records, block_size included, or their concatenation) as [first, end) ranges."""
    recs = _records(records)
    out = []
    for i, r in enumerate(recs):
        if i == 0 or _name(r) != _name(recs[i - 1]):
            out.append([i, i + 1])
        else:
            out[-1][1] = i + 1
    return [tuple(t) for t in out]


def unclipped_5p(rec: bytes) -> int:
    """Rule 3: the unclipped 5' coordinate (0-based) of a mapped record."""
    (rid, pos, l_name, n_cig, flag) = struct.unpack_from("<iiBxxxHH", rec, 4)
    ops = [(c >> 4, c & 15) for c in struct.unpack_from("<%dI" % n_cig, rec, 36 + l_name)]
    def clip(seq):                                        # the S and H lengths before the first other op
        return sum(n for n, _ in itertools.takewhile(lambda x: x[1] in (4, 5), seq))
    if flag & 0x10:
        rlen = sum(n for n, o in ops if o in (0, 2, 3, 7, 8)) or 1
        return pos + rlen - 1 + clip(reversed(ops))
    return pos - clip(ops)


def score(rec: bytes) -> int:
    """Rule 4: the sum of QUAL values >= 15, capped at 16383; 0 when QUAL is absent."""
    (l_name, n_cig, _flag_, l_seq) = struct.unpack_from("<BxxxHHi", rec, 12)
    q0 = 36 + l_name + 4 * n_cig + (l_seq + 1) // 2
    qual = rec[q0:q0 + l_seq]
    if not qual or qual[0] == 0xFF:
        return 0
    return min(sum(q for q in qual if q >= QUAL_MIN), SCORE_CAP)


def ends(records):
    """Rules 1-5 over one batch: (n_templates, the ends of the templates that have one in template order, each record's template)."""
    recs = _records(records)
    tmpls = templates(recs)
    out, rec_tmpl, faults = [], [], []
    for t, (a, b) in enumerate(tmpls):
        rec_tmpl += [t] * (b - a)
        seg, paired, fault = {}, None, None
        for r in range(a, b):
            f = _flag(recs[r])
            if f & 0x900:
                continue
            p = f & 1
            if paired is None:
                paired = p
            if p != paired:
                fault = (r, 2)
            elif p and bool(f & 0x40) == bool(f & 0x80):
                fault = (r, 1)
            else:
                s = "only" if not p else "first" if f & 0x40 else "last"
                if s in seg:
                    fault = (r, 0)
                elif not f & 4 and (struct.unpack_from("<i", recs[r], 4)[0] < 0 or not -(1 << 31) <= unclipped_5p(recs[r]) < 1 << 31):
                    fault = (r, 3)
                else:
                    seg[s] = r
            if fault:
                break
        if fault:
            faults.append(fault)
            continue
        mapped = {s: r for s, r in seg.items() if not _flag(recs[r]) & 4}

        def half(r):
            rec = recs[r]
            return (struct.unpack_from("<i", rec, 4)[0], unclipped_5p(rec), _flag(rec) >> 4 & 1, score(rec))
        if "first" in mapped and "last" in mapped:
            x, y = sorted((mapped["first"], mapped["last"]))
            e1, e2 = half(x), half(y)
            if (e2[0], e2[1]) < (e1[0], e1[1]):
                e1, e2 = e2, e1
            out.append(dict(tmpl=t, ref1=e1[0], pos1=e1[1], ref2=e2[0], pos2=e2[1], score=e1[3] + e2[3], strands=e1[2] | e2[2] << 1))
        elif len(mapped) == 1:
            e1 = half(next(iter(mapped.values())))
            out.append(dict(tmpl=t, ref1=e1[0], pos1=e1[1], ref2=-1, pos2=0, score=e1[3], strands=e1[2]))
    if faults:
        raise MarkdupRefusal(*min(faults))
    return len(tmpls), out, rec_tmpl


def decide(ends_, n_templates: int):
    """Rule 6 over ends (dicts, or rows with the same fields) of templates [0, n_templates): (dup: list of bools, counts)."""
    es = [{k: int(e[k]) for k in ("tmpl", "ref1", "pos1", "ref2", "pos2", "score", "strands")} for e in ends_]
    dup = [False] * n_templates
    pairs, frags = {}, {}
    for e in es:
        rank = (-e["score"], e["tmpl"])
        k1 = (e["ref1"], e["pos1"], e["strands"] & 1)
        if e["ref2"] >= 0:
            pairs.setdefault(k1 + (e["ref2"], e["pos2"], e["strands"] >> 1 & 1), []).append((rank, e["tmpl"]))
            frags.setdefault(k1, []).append((None, e["tmpl"]))
            frags.setdefault((e["ref2"], e["pos2"], e["strands"] >> 1 & 1), []).append((None, e["tmpl"]))
        else:
            frags.setdefault(k1, []).append((rank, e["tmpl"]))
    n_pair_dup = n_frag_dup = 0
    for group in pairs.values():
        for _, t in sorted(group)[1:]:
            dup[t] = True
            n_pair_dup += 1
    for group in frags.values():
        unpaired = sorted(g for g in group if g[0] is not None)
        losers = unpaired if len(unpaired) < len(group) else unpaired[1:]
        for _, t in losers:
            dup[t] = True
            n_frag_dup += 1
    n_pairs = sum(e["ref2"] >= 0 for e in es)
    counts = dict(templates=n_templates, unpaired_examined=len(es) - n_pairs, unpaired_duplicates=n_frag_dup, pairs_examined=n_pairs,
                  pair_duplicates=n_pair_dup, records_marked=0)
    return dup, counts


def percent_duplication(counts: dict) -> float:
    """Picard's PERCENT_DUPLICATION of rule 8's counts."""
    den = counts["unpaired_examined"] + 2 * counts["pairs_examined"]
    return (counts["unpaired_duplicates"] + 2 * counts["pair_duplicates"]) / den if den else 0.0


def set_dup(rec: bytes, on: bool) -> bytes:
    """rec with FLAG 0x400 set (on) or cleared: the only byte rule 7 changes."""
    f = _flag(rec) & ~0x400 | (0x400 if on else 0)
    return rec[:18] + struct.pack("<H", f) + rec[20:]


def mark(runs):
    """Rules 1-8 over runs (records per batch or sorter put, in seq order) as one input: (marked records per run, counts)."""
    per_run, all_ends, base = [], [], 0
    for run in runs:
        recs = _records(run)
        n_t, es, rt = ends(recs)
        all_ends += [dict(e, tmpl=e["tmpl"] + base) for e in es]
        per_run.append((recs, [t + base for t in rt]))
        base += n_t
    dup, counts = decide(all_ends, base)
    out = []
    for recs, rt in per_run:
        marked = [set_dup(r, dup[t]) for r, t in zip(recs, rt)]
        counts["records_marked"] += sum(dup[t] for t in rt)
        out.append(b"".join(marked))
    counts["percent_duplication"] = percent_duplication(counts)
    return out, counts
