"""Duplicate marking restated in Python: the yardstick of csrc/markdup.hip and of the sorter's BWAMS_SORT_MARKDUP.

These are Picard MarkDuplicates' rules for query-grouped input: default SUM_OF_BASE_QUALITIES scoring, no barcodes.  Rules 1-8 are
one library without optical duplicate detection; rules 9-15 add read groups, libraries, optical duplicates and the metrics file.
Neither Picard nor samtools is a dependency, so the rules below are the specification:

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

9. Read groups and libraries.  A groups table is made from SAM header text.  Every @RG line gives a read group; its ordinal is the
   line's place among the @RG lines.  Its ID is required: a line without one, or two lines with one ID, is refused (ValueError;
   BWAMS_ERR_ARG).  Its LB is optional.  Libraries are the distinct LB values in order of first appearance, ordinals from 0; after
   them comes one more, "Unknown Library", which always exists, so n_lib = distinct LBs + 1.  With no table n_lib = 1 and everything
   is "Unknown Library".  A record's read group is the value of its first aux field with tag RG and type Z, found by walking the aux
   fields by their types (SAMv1 4.2.4: A c C s S i I f Z H B) to the record's end.  A field of unknown type (or a B array of unknown
   element type), or one that runs past block_size, refuses the batch as rules 2-3 do, with a fifth reason, "aux fields do not chain
   to the record's end"; rules 2-3 are checked over the whole batch first, so this reason names the first such record of a batch
   they accept.  Only one record per template is walked: its first primary in record order, or its first record when it has no primary; and only when a
   table is given.  That record's read group is the template's; ordinal -1 means no RG field or a value not in the table.  The
   template's library is its read group's; ordinal -1 and read groups without LB belong to "Unknown Library".
10. Location, from the name of the record rule 9 names (without its NUL), split at ':'.  Exactly 5 fields: tile, x, y are fields 2, 3,
   4 (from 0).  Exactly 7 or 8 fields: fields 4, 5, 6.  Any other count: no location.  A field's value is an optional '-', then the
   decimal digits up to the first byte that is not a digit; the rest is ignored and no digits gives 0.  A value outside int32 means
   no location.
11. Keys.  The library ordinal is the most significant part of the pair key and of the fragment key of rules 5-6: equal places in two
   libraries are not duplicates of each other.
12. Optical duplicates, for a distance d > 0 (Picard's default is 100, and 2500 for patterned flow cells; 0 turns it off).  Only
   pairs are examined.  In a group of pairs with equal key that holds between 2 and max_set members (Picard: 300000), two members are
   close when both have a location, their read-group ordinals are equal (-1 equals -1), their tiles are equal, and |x - x'| <= d and
   |y - y'| <= d.  Clusters are the connected components of "close"; a member with no location is a cluster of its own.  A cluster's
   representative is the group's kept pair (rule 6) if it is in the cluster, otherwise the member with the smallest template
   ordinal.  Every other member is an optical duplicate, so a group's optical count is the sum over its clusters of (size - 1).
   (Picard switches between two algorithms at a group size of 4; both give this count.)  Nothing is written into the records.
13. Per-library counts, each attributed to the template's library: unpaired_examined, pairs_examined, unpaired_duplicates,
   pair_duplicates as in rule 8; pair_optical_duplicates: rule 12; secondary_or_supplementary: records with 0x100 or 0x800 set and
   0x4 clear; unmapped: records with 0x4 set; percent_duplication: rule 8's formula, 0 when the denominator is 0;
   estimated_library_size: rule 14, -1 for none.  Summed over libraries, the first four equal rule 8's.
14. Estimated library size: Picard's estimateLibrarySize in doubles.  n = pairs_examined - pair_optical_duplicates, c =
   pairs_examined - pair_duplicates.  None if n <= 0, n - c <= 0 or c <= 0.  Otherwise, with f(x) = c/x - 1 + exp(-n/x): m = 1.0,
   M = 100.0; while f(M*c) > 0: M *= 10.0; 40 times: r = (m + M) / 2, u = f(r*c), stop if u == 0, m = r if u > 0 else M = r; the
   result is int(c * (m + M) / 2.0).
15. Metrics text, Picard's layout: "## htsjdk.samtools.metrics.StringHeader"; "# " and the caller's text; "## METRICS CLASS<tab>
   picard.sam.DuplicationMetrics"; the column line; one row per library that has any count above zero, in ordinal order; an empty
   line.  PERCENT_DUPLICATION is printed as %.6f; ESTIMATED_LIBRARY_SIZE is left empty when there is none.  Picard's histogram
   section is not written.

Templates joined by name (bwams_dupjoin_t, csrc/dup_join.hip): duplicate marking of records that are not query-grouped, such as a
coordinate-sorted BAM.  Rules 2 to 15 hold unchanged except where a rule below says otherwise.  "Add order" is the order of the adds,
then record order within each; a record's ordinal is its 0-based place in add order.

J1. Name key.  L = l_read_name - 1, the name without its NUL.  For each of two seeds S0 = 0x9e3779b97f4a7c15 and S1 =
    0xc2b2ae3d27d4eb4f: h = S ^ L; then for i in [0, max(1, ceil(L / 8))): h = fmix64(h ^ w_i), where w_i is the name's bytes
    [8i, 8i + 8) as a little-endian 64-bit word, zero-padded past L, and fmix64 is MurmurHash3's finalizer (h ^= h >> 33; h *=
    0xff51afd7ed558ccd; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53; h ^= h >> 33; mod 2^64).  The key is (k0, k1).  Names of at most 8
    bytes cannot collide within one length: one bijective step.
J2. Template: all added records with equal (L, k0, k1), adjacent or not.  This replaces rule 1.  Its ordinal is its rank by the
    ordinal of its first record.  Two different names with equal L and key would be taken for one template (among 2^32 names the
    chance of any such pair is below 2^-65); the consequence is a wrong 0x400 or a refusal by rule 2.  More than 2^32 - 1 records
    are refused.
J3. The walk.  Rules 2 to 5 are applied to a template's records in ordinal order: "the earlier record" of rule 5 is the one with
    the smaller ordinal, "the first record concerned" of rule 2 the smallest ordinal at which any template's walk meets a fault.
    So two primaries of one segment that share a name are refused wherever they lie; the adjacent-run rule takes them for two
    templates when they are apart.
J4. Read group, library, location.  Rules 9 and 10 take the template's first primary in add order, or its first record when it has no
    primary.  With a groups table every added record's aux fields are walked at the add; a record that does not chain refuses that
    add (MarkdupRefusal with reason AUX, naming the smallest such ordinal), before rules 2-3 are looked at.  Without a table no aux
    field is read.
J5. Decision and tie-breaks.  Rule 6 and rules 11 to 13 apply; "earlier template" means the smaller template ordinal of J2.
J6. Marking.  Rule 7 applies: every record of a duplicate template is marked, secondary, supplementary and unmapped-mate records
    included, wherever they lie.  This is what the query-grouped path does, and more than Picard does on coordinate-sorted input.
J7. Defined over what was added.  A paired primary whose mate was never added makes a fragment; the whole file is the intended input.
J8. Pass 2 (the library only): apply call i takes the records of add i, checked by their count and two sums of their k0.
J9. States (the library only): empty -> adding -> finished.

name_key(name) -> (k0, k1); join(adds, table) -> (n_templates, ends, rec_tmpl by ordinal, locs parallel to ends, each template's
library); mark_joined(adds, header_text, distance, max_set) -> (marked records per add, rule 8's counts, rule 13's rows).

groups(header_text) -> Groups (rule 9); read_group(rec) -> the RG:Z value or None; location(name) -> (tile, x, y) or None;
ends2(records, groups) -> ends' (n_templates, ends, rec_tmpl, locs, each template's library); decide2(ends, locs, n_templates, n_lib,
distance, max_set) -> (dup, optical, per-library rows); mark2(runs, header_text, distance, max_set) -> (marked records per run,
counts, rows); estimate_library_size(n, c); metrics_text(groups, rows, comment).  A loc is a dict with the fields of bwams_dup_loc_t.
The optical clusters are written in the plainest way, all pairs of a group and then components, which is not the kernel's way.

templates(records) -> [(first, end)] (rule 1); ends(records) -> (n_templates, ends, rec_tmpl), refusing with MarkdupRefusal;
decide(ends, n_templates) -> (dup per template, counts); mark(runs) -> (marked records per run, counts), runs in seq order.
An end is a dict with the fields of bwams_dup_end_t: tmpl, ref1, pos1, ref2 (-1 for a fragment), pos2, score, strands.
"""
from __future__ import annotations

import itertools
import math
import struct

from .bam import split_records

QUAL_MIN, SCORE_CAP = 15, 16383
REASONS = ("two primaries of one segment", "a paired primary with neither or both of 0x40 / 0x80",
           "paired and unpaired primaries mixed", "a mapped primary's unclipped 5' coordinate outside [-2^31, 2^31) or its refID -1",
           "aux fields do not chain to the record's end")
AUX = 4                                                  # rule 9's reason
UNKNOWN_LIBRARY = "Unknown Library"
MAX_SET = 300000
LIB_COUNTS = ("unpaired_examined", "pairs_examined", "secondary_or_supplementary", "unmapped", "unpaired_duplicates", "pair_duplicates",
              "pair_optical_duplicates")
COLUMNS = ("LIBRARY", "UNPAIRED_READS_EXAMINED", "READ_PAIRS_EXAMINED", "SECONDARY_OR_SUPPLEMENTARY_RDS", "UNMAPPED_READS",
           "UNPAIRED_READ_DUPLICATES", "READ_PAIR_DUPLICATES", "READ_PAIR_OPTICAL_DUPLICATES", "PERCENT_DUPLICATION",
           "ESTIMATED_LIBRARY_SIZE")


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


# ---- rules 9-15 ----

class Groups:
    """Rule 9's table: ids (bytes) by read-group ordinal, rg_lib their library ordinals, libs the libraries' names (str)."""

    def __init__(self, ids, rg_lib, libs):
        self.ids, self.rg_lib, self.libs = ids, rg_lib, libs
        self.n_lib = len(libs)

    def lib_of(self, rg: int) -> int:
        return self.rg_lib[rg] if rg >= 0 else self.n_lib - 1


def groups(header_text) -> Groups:
    """Rule 9: the groups table of SAM header text (bytes or str); ValueError for an @RG line without ID or a repeated ID."""
    text = header_text.encode() if isinstance(header_text, str) else bytes(header_text)
    ids, lbs = [], []
    for line in text.split(b"\n"):
        if line.endswith(b"\r"):
            line = line[:-1]
        f = line.split(b"\t")
        if f[0] != b"@RG":
            continue
        tags = {}
        for x in f[1:]:
            if len(x) >= 3 and x[2:3] == b":":
                tags.setdefault(x[:2], x[3:])
        if b"ID" not in tags or tags[b"ID"] in ids:
            raise ValueError("@RG line without ID, or two with one ID")
        ids.append(tags[b"ID"])
        lbs.append(tags.get(b"LB"))
    libs = []
    for lb in lbs:
        if lb is not None and lb not in libs:
            libs.append(lb)
    rg_lib = [libs.index(lb) if lb is not None else len(libs) for lb in lbs]
    return Groups(ids, rg_lib, [x.decode("latin-1") for x in libs] + [UNKNOWN_LIBRARY])


_AUX_SIZE = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}


def read_group(rec: bytes):
    """Rule 9: the value of rec's first RG:Z aux field (bytes) or None; ValueError when the aux fields do not chain to the end."""
    (l_name, n_cig, _f, l_seq) = struct.unpack_from("<BxxxHHi", rec, 12)
    n = 4 + struct.unpack_from("<I", rec, 0)[0]
    a = 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    if l_seq < 0 or a > n or n > len(rec):
        raise ValueError(REASONS[AUX])
    found = None
    while a < n:
        if a + 3 > n:
            raise ValueError(REASONS[AUX])
        tag, ty = rec[a:a + 2], rec[a + 2:a + 3]
        a += 3
        if ty in (b"Z", b"H"):
            e = rec.find(b"\0", a, n)
            if e < 0:
                raise ValueError(REASONS[AUX])
            if ty == b"Z" and tag == b"RG" and found is None:
                found = rec[a:e]
            a = e + 1
        elif ty == b"B":
            if a + 5 > n or rec[a:a + 1] == b"A" or rec[a:a + 1] not in _AUX_SIZE:
                raise ValueError(REASONS[AUX])
            a += 5 + _AUX_SIZE[rec[a:a + 1]] * struct.unpack_from("<I", rec, a + 1)[0]
        elif ty in _AUX_SIZE:
            a += _AUX_SIZE[ty]
        else:
            raise ValueError(REASONS[AUX])
        if a > n:
            raise ValueError(REASONS[AUX])
    return found


def _value(field: bytes) -> int:
    neg = field[:1] == b"-"
    digits = field[1:] if neg else field
    k = 0
    while k < len(digits) and 48 <= digits[k] <= 57:
        k += 1
    v = int(digits[:k]) if k else 0
    return -v if neg else v


def location(name: bytes):
    """Rule 10: (tile, x, y) of a read name (without its NUL), or None."""
    f = bytes(name).split(b":")
    first = {5: 2, 7: 4, 8: 4}.get(len(f))
    if first is None:
        return None
    v = tuple(_value(x) for x in f[first:first + 3])
    return v if all(-(1 << 31) <= x < 1 << 31 for x in v) else None


def ends2(records, table: Groups | None):
    """Rules 1-5 and 9-10 over one batch: (n_templates, ends, rec_tmpl, locs parallel to ends, each template's library).  The aux
    fields are walked only with a table; its refusal is MarkdupRefusal(record, AUX)."""
    recs = _records(records)
    n_t, es, rt = ends(recs)                                         # rules 2-3 refuse first
    tmpls = templates(recs)
    faults, tloc = [], []
    n_lib = table.n_lib if table else 1
    for a, b in tmpls:
        r = next((r for r in range(a, b) if not _flag(recs[r]) & 0x900), a)
        rg = -1
        if table:
            try:
                v = read_group(recs[r])
                rg = table.ids.index(v) if v in table.ids else -1
            except ValueError:
                faults.append((r, AUX))
        name = recs[r][36:36 + max(recs[r][12] - 1, 0)]
        at = location(name)
        tile, x, y = at if at else (0, 0, 0)
        tloc.append(dict(lib=table.lib_of(rg) if table else n_lib - 1, rg=rg, tile=tile, x=x, y=y, has=int(at is not None)))
    if faults:
        raise MarkdupRefusal(*min(faults))
    return n_t, es, rt, [tloc[e["tmpl"]] for e in es], [t["lib"] for t in tloc]


def estimate_library_size(n: int, c: int):
    """Rule 14: Picard's estimateLibrarySize, None for none."""
    if n <= 0 or n - c <= 0 or c <= 0:
        return None
    n, c = float(n), float(c)
    f = lambda x: c / x - 1.0 + math.exp(-n / x)                     # noqa: E731
    m, M = 1.0, 100.0
    while f(M * c) > 0:
        M *= 10.0
    for _ in range(40):
        r = (m + M) / 2.0
        u = f(r * c)
        if u == 0:
            break
        if u > 0:
            m = r
        else:
            M = r
    return int(c * (m + M) / 2.0)


def finish_row(row: dict) -> dict:
    """Rule 13's percent_duplication and estimated_library_size (-1 for none) from the row's counts."""
    row["percent_duplication"] = percent_duplication(row)
    size = estimate_library_size(row["pairs_examined"] - row["pair_optical_duplicates"], row["pairs_examined"] - row["pair_duplicates"])
    row["estimated_library_size"] = -1 if size is None else size
    return row


def decide2(ends_, locs, n_templates: int, n_lib: int = 1, distance: int = 0, max_set: int = MAX_SET):
    """Rules 6 and 11-13 over ends and their locs (None: library 0, no location): (dup, optical: lists of bools per template, rows:
    one dict per library, the two record-level counts 0)."""
    es = [{k: int(e[k]) for k in ("tmpl", "ref1", "pos1", "ref2", "pos2", "score", "strands")} for e in ends_]
    ls = [dict(lib=0, rg=-1, tile=0, x=0, y=0, has=0) for _ in es] if locs is None else \
        [{k: int(l[k]) for k in ("lib", "rg", "tile", "x", "y", "has")} for l in locs]
    for i, l in enumerate(ls):
        if not 0 <= l["lib"] < n_lib or l["has"] not in (0, 1):
            raise ValueError("end %d: loc.lib outside [0, n_lib) or loc.has outside {0, 1}" % i)
    dup, optical = [False] * n_templates, [False] * n_templates
    pairs = {}                                                       # rule 11: a library is a world of its own
    for lib in range(n_lib):
        sub = [e for e, l in zip(es, ls) if l["lib"] == lib]
        d, _ = decide(sub, n_templates)
        dup = [a or b for a, b in zip(dup, d)]
    for e, l in zip(es, ls):
        if e["ref2"] >= 0:
            key = (l["lib"], e["ref1"], e["pos1"], e["strands"] & 1, e["ref2"], e["pos2"], e["strands"] >> 1 & 1)
            pairs.setdefault(key, []).append((e, l))
    if distance > 0:
        for group in pairs.values():
            if not 2 <= len(group) <= max_set:
                continue
            n = len(group)
            near = lambda a, b: (a["has"] == 1 and b["has"] == 1 and a["rg"] == b["rg"] and a["tile"] == b["tile"] and   # noqa: E731
                                 abs(a["x"] - b["x"]) <= distance and abs(a["y"] - b["y"]) <= distance)
            close = [[j for j in range(n) if j != i and near(group[i][1], group[j][1])] for i in range(n)]     # all pairs
            comp = [-1] * n                                          # components: flood from every member not yet reached
            for i in range(n):
                if comp[i] >= 0:
                    continue
                comp[i], todo = i, [i]
                while todo:
                    for j in close[todo.pop()]:
                        if comp[j] < 0:
                            comp[j] = i
                            todo.append(j)
            for c in set(comp):
                members = [group[i][0]["tmpl"] for i in range(n) if comp[i] == c]
                kept = [t for t in members if not dup[t]]            # the group's kept pair, if it is in this cluster
                rep = kept[0] if kept else min(members)
                for t in members:
                    optical[t] = t != rep
    rows = [dict.fromkeys(LIB_COUNTS, 0) for _ in range(n_lib)]
    for e, l in zip(es, ls):
        row, pair = rows[l["lib"]], e["ref2"] >= 0
        row["pairs_examined" if pair else "unpaired_examined"] += 1
        if dup[e["tmpl"]]:
            row["pair_duplicates" if pair else "unpaired_duplicates"] += 1
        row["pair_optical_duplicates"] += optical[e["tmpl"]]
    return dup, optical, [finish_row(r) for r in rows]


def mark2(runs, header_text=None, distance: int = 0, max_set: int = MAX_SET):
    """Rules 1-14 over runs (in seq order) as one input: (marked records per run, rule 8's counts, rule 13's rows)."""
    table = groups(header_text) if header_text is not None else None
    n_lib = table.n_lib if table else 1
    per_run, all_ends, all_locs, base = [], [], [], 0
    rec_counts = [[0, 0] for _ in range(n_lib)]
    for run in runs:
        recs = _records(run)
        n_t, es, rt, locs, tlib = ends2(recs, table)
        all_ends += [dict(e, tmpl=e["tmpl"] + base) for e in es]
        all_locs += locs
        per_run.append((recs, [t + base for t in rt]))
        for r, t in zip(recs, rt):
            f = _flag(r)
            if f & 4:
                rec_counts[tlib[t]][1] += 1
            elif f & 0x900:
                rec_counts[tlib[t]][0] += 1
        base += n_t
    dup, _optical, rows = decide2(all_ends, all_locs, base, n_lib, distance, max_set)
    for row, (ss, un) in zip(rows, rec_counts):
        row["secondary_or_supplementary"], row["unmapped"] = ss, un
    counts = dict(templates=base, records_marked=0)
    for k in ("unpaired_examined", "unpaired_duplicates", "pairs_examined", "pair_duplicates"):
        counts[k] = sum(r[k] for r in rows)
    out = []
    for recs, rt in per_run:
        out.append(b"".join(set_dup(r, dup[t]) for r, t in zip(recs, rt)))
        counts["records_marked"] += sum(dup[t] for t in rt)
    counts["percent_duplication"] = percent_duplication(counts)
    return out, counts, rows


def metrics_text(table: Groups | None, rows, comment: str = "") -> str:
    """Rule 15: the DuplicationMetrics text of rule 13's rows."""
    libs = table.libs if table else [UNKNOWN_LIBRARY]
    out = ["## htsjdk.samtools.metrics.StringHeader", "# " + comment, "## METRICS CLASS\tpicard.sam.DuplicationMetrics", "\t".join(COLUMNS)]
    for name, r in zip(libs, rows):
        if not any(r[k] > 0 for k in LIB_COUNTS):
            continue
        size = r["estimated_library_size"]
        out.append("\t".join([name] + [str(r[k]) for k in LIB_COUNTS] + ["%.6f" % r["percent_duplication"], "" if size < 0 else str(size)]))
    return "\n".join(out) + "\n\n"


# ---- templates joined by name: rules J1-J9 ----

JOIN_SEEDS = (0x9e3779b97f4a7c15, 0xc2b2ae3d27d4eb4f)
_M64 = (1 << 64) - 1


def _fmix64(h: int) -> int:
    h ^= h >> 33
    h = h * 0xff51afd7ed558ccd & _M64
    h ^= h >> 33
    h = h * 0xc4ceb9fe1a85ec53 & _M64
    return h ^ h >> 33


def name_key(name) -> tuple[int, int]:
    """J1: (k0, k1) of a read name (bytes, without its NUL)."""
    name = bytes(name)
    out = []
    for seed in JOIN_SEEDS:
        h = seed ^ len(name)
        for i in range(max(1, (len(name) + 7) // 8)):
            h = _fmix64(h ^ int.from_bytes(name[8 * i:8 * i + 8], "little"))
        out.append(h)
    return out[0], out[1]


def join(adds, table: Groups | None = None):
    """J1-J4 over adds (records per add, in add order): (n_templates, the ends of the templates that have one in template order,
    each record's template by ordinal, locs parallel to ends, each template's library), refusing with MarkdupRefusal."""
    recs = []
    for add in adds:
        piece = _records(add)
        if table:                                                    # J4: every record of the add is walked, and refuses that add
            for k, r in enumerate(piece):
                try:
                    read_group(r)
                except ValueError:
                    raise MarkdupRefusal(len(recs) + k, AUX) from None
        recs += piece
    by_key = {}                                                      # J2: insertion order is the order of the first records
    for o, r in enumerate(recs):
        name = r[36:36 + max(r[12] - 1, 0)]
        by_key.setdefault((len(name),) + name_key(name), []).append(o)
    n_lib = table.n_lib if table else 1
    out, rec_tmpl, faults, tloc = [], [0] * len(recs), [], []
    for t, members in enumerate(by_key.values()):
        seg, paired, fault = {}, None, None
        for o in members:                                            # J3: rules 2-5 in ordinal order
            rec_tmpl[o] = t
            f = _flag(recs[o])
            if fault or f & 0x900:
                continue
            p = f & 1
            if paired is None:
                paired = p
            if p != paired:
                fault = (o, 2)
            elif p and bool(f & 0x40) == bool(f & 0x80):
                fault = (o, 1)
            else:
                s = "only" if not p else "first" if f & 0x40 else "last"
                if s in seg:
                    fault = (o, 0)
                elif not f & 4 and (struct.unpack_from("<i", recs[o], 4)[0] < 0 or not -(1 << 31) <= unclipped_5p(recs[o]) < 1 << 31):
                    fault = (o, 3)
                else:
                    seg[s] = o
        named = next((o for o in members if not _flag(recs[o]) & 0x900), members[0])      # J4
        rg = -1
        if table:
            v = read_group(recs[named])
            rg = table.ids.index(v) if v in table.ids else -1
        at = location(recs[named][36:36 + max(recs[named][12] - 1, 0)])
        tile, x, y = at if at else (0, 0, 0)
        tloc.append(dict(lib=table.lib_of(rg) if table else n_lib - 1, rg=rg, tile=tile, x=x, y=y, has=int(at is not None)))
        if fault:
            faults.append(fault)
            continue
        mapped = {s: o for s, o in seg.items() if not _flag(recs[o]) & 4}

        def half(o):
            rec = recs[o]
            return (struct.unpack_from("<i", rec, 4)[0], unclipped_5p(rec), _flag(rec) >> 4 & 1, score(rec))
        if "first" in mapped and "last" in mapped:
            e1, e2 = (half(o) for o in sorted((mapped["first"], mapped["last"])))
            if (e2[0], e2[1]) < (e1[0], e1[1]):
                e1, e2 = e2, e1
            out.append(dict(tmpl=t, ref1=e1[0], pos1=e1[1], ref2=e2[0], pos2=e2[1], score=e1[3] + e2[3], strands=e1[2] | e2[2] << 1))
        elif len(mapped) == 1:
            e1 = half(next(iter(mapped.values())))
            out.append(dict(tmpl=t, ref1=e1[0], pos1=e1[1], ref2=-1, pos2=0, score=e1[3], strands=e1[2]))
    if faults:
        raise MarkdupRefusal(*min(faults))
    return len(by_key), out, rec_tmpl, [tloc[e["tmpl"]] for e in out], [t["lib"] for t in tloc]


def mark_joined(adds, header_text=None, distance: int = 0, max_set: int = MAX_SET):
    """J1-J7 over adds as one input: (marked records per add, rule 8's counts, rule 13's rows)."""
    table = groups(header_text) if header_text is not None else None
    n_lib = table.n_lib if table else 1
    pieces = [_records(a) for a in adds]
    n_t, es, rt, locs, tlib = join(pieces, table)
    dup, _optical, rows = decide2(es, locs, n_t, n_lib, distance, max_set)
    flat = [r for piece in pieces for r in piece]
    for r, t in zip(flat, rt):
        f = _flag(r)
        if f & 4:
            rows[tlib[t]]["unmapped"] += 1
        elif f & 0x900:
            rows[tlib[t]]["secondary_or_supplementary"] += 1
    counts = dict(templates=n_t, records_marked=sum(dup[t] for t in rt))
    for k in ("unpaired_examined", "unpaired_duplicates", "pairs_examined", "pair_duplicates"):
        counts[k] = sum(r[k] for r in rows)
    counts["percent_duplication"] = percent_duplication(counts)
    out, base = [], 0
    for piece in pieces:
        out.append(b"".join(set_dup(r, dup[t]) for r, t in zip(piece, rt[base:base + len(piece)])))
        base += len(piece)
    return out, counts, rows
