"""Duplicate marking's rules 9-15 (include/bwams.h above bwams_bam_templates: read groups and libraries, locations, optical duplicates,
per-library counts, the estimated library size and the metrics text): bwams/markdup.py against expectations written out here.
tests/test_gpu_markdup_metrics.py runs the same cases through bwams_bam_templates2, bwams_dup_decide2 and bwams_bam_markdup2."""
import struct

import pytest

from bwams import markdup
from test_markdup import CASES, D, P1, P2, R, flags, rec


def with_aux(r: bytes, aux: bytes) -> bytes:
    """the record r with aux appended and block_size to match"""
    body = r[4:] + aux
    return struct.pack("<I", len(body)) + body


def rgz(rg) -> bytes:
    return b"" if rg is None else b"RGZ" + rg + b"\0"


def pair(name: bytes, qual: bytes = b"I", rg=None, at=(300, 500)) -> list:
    """an FR pair at fixed places: the first end forward at at[0], the last reverse at at[1]; both records carry RG:Z:rg"""
    return [with_aux(rec(name, P1, at[0], qual=qual), rgz(rg)), with_aux(rec(name, P2 | R, at[1], qual=qual), rgz(rg))]


def frag(name: bytes, qual: bytes = b"I", rg=None, at=300) -> list:
    return [with_aux(rec(name, 0, at, qual=qual), rgz(rg))]


# ---- rule 9: the groups table ----

H_ONE_LIB = "@HD\tVN:1.6\tSO:unsorted\n@RG\tID:a\tSM:s\tLB:L\tPL:ILLUMINA\n@RG\tID:b\tLB:L\n"
H_TWO_LIBS = "@RG\tID:a\tLB:L1\n@RG\tLB:L2\tID:c\n"
H_NO_LB = "@RG\tID:solo\tSM:x\r\n"
H_NO_RG = "@HD\tVN:1.6\n@SQ\tSN:c0\tLN:1000\n@SQ\tSN:c1\tLN:1000\n@PG\tID:bwa\tPN:bwa\tCL:mem -R @RG\\tID:z\n"
# (case, header text, ids, each read group's library, the libraries)
GROUPS = [
    ("two_rg_one_lb", H_ONE_LIB, [b"a", b"b"], [0, 0], ["L", "Unknown Library"]),
    ("two_libs", H_TWO_LIBS, [b"a", b"c"], [0, 1], ["L1", "L2", "Unknown Library"]),
    ("no_lb", H_NO_LB, [b"solo"], [0], ["Unknown Library"]),
    ("no_rg_line", H_NO_RG, [], [], ["Unknown Library"]),
    ("lb_after_none", "@RG\tID:x\n@RG\tID:y\tLB:late\n", [b"x", b"y"], [1, 0], ["late", "Unknown Library"]),
]
GROUPS_REFUSED = [("duplicate_id", "@RG\tID:a\tLB:L\n@RG\tID:a\tLB:M\n"), ("no_id", "@RG\tLB:L\n")]


@pytest.mark.parametrize("case", GROUPS, ids=[c[0] for c in GROUPS])
def test_groups(case):
    _, text, ids, rg_lib, libs = case
    g = markdup.groups(text)
    assert (g.ids, g.rg_lib, g.libs, g.n_lib) == (ids, rg_lib, libs, len(libs))
    assert markdup.groups(text.encode()).libs == libs


@pytest.mark.parametrize("case", GROUPS_REFUSED, ids=[c[0] for c in GROUPS_REFUSED])
def test_groups_refused(case):
    with pytest.raises(ValueError):
        markdup.groups(case[1])


# ---- rule 9: the walk over the aux fields ----

EVERY_TYPE = (b"XAAx" + b"Xcc\xff" + b"XCC\x01" + b"Xss\x01\x02" + b"XSS\x01\x02" + b"Xii\x01\x02\x03\x04" + b"XII\x01\x02\x03\x04" +
              b"Xff\0\0\x80\x3f" + b"XZZRG:Z:no\0" + b"XHH1AE3\0" + b"XBBs\x03\0\0\0abcdef" + b"XbBf\x01\0\0\0\0\0\x80\x3f" +
              b"XcBC\0\0\0\0")
# (case, the aux bytes, the read group's value: None for none, REFUSED for a refusal with the fifth reason)
REFUSED = "refused"
WALKS = [
    ("no_aux", b"", None),
    ("behind_every_type", EVERY_TYPE + b"RGZgrp1\0", b"grp1"),
    ("rg_last_to_block_size", b"NMi\x02\0\0\0RGZa\0", b"a"),
    ("rg_of_type_A_ignored", b"RGAx" + b"RGZreal\0", b"real"),
    ("only_rg_of_type_A", b"RGAx", None),
    ("first_of_two", b"RGZone\0RGZtwo\0", b"one"),
    ("empty_value", b"RGZ\0", b""),
    ("truncated_Z", b"RGZabc", REFUSED),
    ("unknown_type", b"XXq\x01", REFUSED),
    ("array_past_end", b"XBBi\x02\0\0\0\x01\0\0\0", REFUSED),
    ("array_of_unknown_type", b"XBBZ\0\0\0\0", REFUSED),
    ("half_a_field", b"RG", REFUSED),
    ("fault_behind_rg", b"RGZa\0XSS\x01", REFUSED),
]


@pytest.mark.parametrize("case", WALKS, ids=[c[0] for c in WALKS])
def test_read_group(case):
    _, aux, want = case
    r = with_aux(rec(b"n", 0, 10), aux)
    if want is REFUSED:
        with pytest.raises(ValueError, match="aux fields do not chain to the record's end"):
            markdup.read_group(r)
        with pytest.raises(markdup.MarkdupRefusal) as e:
            markdup.mark2([rec(b"ok", 0, 5) + r], H_ONE_LIB)
        assert (e.value.record, e.value.reason) == (1, markdup.AUX)
        assert str(e.value) == "record 1: aux fields do not chain to the record's end"
        markdup.mark2([rec(b"ok", 0, 5) + r], None)                  # without a table nothing is walked
    else:
        assert markdup.read_group(r) == want


def test_walked_record_and_template_group():
    """the first primary in record order is the one walked; without a primary, the first record"""
    bad = b"RGZabc"
    recs = [with_aux(rec(b"t", P1 | 0x800, 900, b"20M30H"), bad), with_aux(rec(b"t", P2 | R, 500), rgz(b"b")),
            with_aux(rec(b"t", P1, 300), rgz(b"a")),
            with_aux(rec(b"u", 0x100, 40), rgz(b"a")), with_aux(rec(b"u", 0x100, 50), bad)]
    n_t, es, rt, locs, tlib = markdup.ends2(recs, markdup.groups(H_TWO_LIBS))
    assert (n_t, rt, tlib) == (2, [0, 0, 0, 1, 1], [2, 0])           # b is not in the table: Unknown Library; u: read group a
    assert locs == [dict(lib=2, rg=-1, tile=0, x=0, y=0, has=0)]     # u has no end
    with pytest.raises(markdup.MarkdupRefusal) as e:                   # rules 2-3 refuse first, also at a later record
        markdup.ends2([with_aux(rec(b"x", 0, 5), bad), rec(b"a", 0, 5, ref=b"*")], markdup.groups(H_TWO_LIBS))
    assert (e.value.record, e.value.reason) == (1, 3)


# ---- rule 10: names ----

NAMES = [
    (b"a:b:7:100:200", (7, 100, 200)),                               # 5 fields
    (b"M0:12:FC1:3:1101:15589:1332", (1101, 15589, 1332)),            # 7
    (b"M0:12:FC1:3:1101:15589:1332:ACGT", (1101, 15589, 1332)),       # 8
    (b"a:7:100:200", None), (b"a:b:c:7:100:200", None),               # 4 and 6
    (b"plain", None), (b"a:b:c:d:e:f:g:h:i", None),
    (b"a:b:7:12x:200", (7, 12, 200)), (b"a:b:7::200", (7, 0, 200)), (b"a:b:7:-3:200", (7, -3, 200)),
    (b"a:b:7:100:200/1", (7, 100, 200)), (b"a:b:7:x12:-", (7, 0, 0)), (b"a:b:7:+5:2", (7, 0, 2)),
    (b"a:b:7:2147483647:-2147483648", (7, 2147483647, -2147483648)),
    (b"a:b:7:2147483648:200", None), (b"a:b:7:1:-2147483649", None), (b"a:b:99999999999999999999999:1:2", None),
    (b"::::", (0, 0, 0)),
]


@pytest.mark.parametrize("case", NAMES, ids=[c[0].decode() for c in NAMES])
def test_location(case):
    assert markdup.location(case[0]) == case[1]


# ---- rules 11-13: hand-built templates ----

def nm(tile: int, x: int, y: int, tag: bytes) -> bytes:
    return b"%s:l:%d:%d:%d" % (tag, tile, x, y)


def chain(n: int, step: int, broken=()) -> list:
    """n pairs of one group on one tile, x = step * i (one more step after every i in broken) and y = 7; the first has the best score"""
    out, x = [], 0
    for i in range(n):
        out += pair(nm(1, x, 7, b"c%d" % i), b"I" if i == 0 else b"5", b"a")
        x += step * (2 if i in broken else 1)
    return out


PE = dict(pairs_examined=1)
# (case, header text or None, records, d, max_set, dup per template, optical per template, {library: its counts above zero})
OPTICAL = [
    ("two_at_d", H_ONE_LIB, pair(nm(1, 100, 100, b"A"), rg=b"a") + pair(nm(1, 110, 110, b"B"), b"5", b"a"), 10, 0,
     [0, 1], [0, 1], {0: dict(pairs_examined=2, pair_duplicates=1, pair_optical_duplicates=1)}),
    ("two_x_past_d", H_ONE_LIB, pair(nm(1, 100, 100, b"A"), rg=b"a") + pair(nm(1, 111, 100, b"B"), b"5", b"a"), 10, 0,
     [0, 1], [0, 0], {0: dict(pairs_examined=2, pair_duplicates=1)}),
    ("two_y_past_d", H_ONE_LIB, pair(nm(1, 100, 100, b"A"), rg=b"a") + pair(nm(1, 100, 89, b"B"), b"5", b"a"), 10, 0,
     [0, 1], [0, 0], {0: dict(pairs_examined=2, pair_duplicates=1)}),
    ("distance_off", H_ONE_LIB, pair(nm(1, 100, 100, b"A"), rg=b"a") + pair(nm(1, 100, 100, b"B"), b"5", b"a"), 0, 0,
     [0, 1], [0, 0], {0: dict(pairs_examined=2, pair_duplicates=1)}),
    ("chain_keeper_at_its_end", H_ONE_LIB,                              # A - B - C, A and C not close: one cluster
     pair(nm(1, 100, 5, b"A"), rg=b"a") + pair(nm(1, 110, 5, b"B"), b"5", b"a") + pair(nm(1, 120, 5, b"C"), b"5", b"a"), 10, 0,
     [0, 1, 1], [0, 1, 1], {0: dict(pairs_examined=3, pair_duplicates=2, pair_optical_duplicates=2)}),
    ("chain_keeper_inside", H_ONE_LIB,
     pair(nm(1, 100, 5, b"A"), b"5", b"a") + pair(nm(1, 110, 5, b"B"), b"I", b"a") + pair(nm(1, 120, 5, b"C"), b"5", b"a"), 10, 0,
     [1, 0, 1], [1, 0, 1], {0: dict(pairs_examined=3, pair_duplicates=2, pair_optical_duplicates=2)}),
    ("chain_keeper_outside", H_ONE_LIB,                                 # the chain of three does not hold the kept pair: its first stands for it
     pair(nm(1, 120, 5, b"C"), b"5", b"a") + pair(nm(1, 9000, 5, b"K"), b"I", b"a") + pair(nm(1, 110, 5, b"B"), b"5", b"a") +
     pair(nm(1, 100, 5, b"A"), b"5", b"a"), 10, 0,
     [1, 0, 1, 1], [0, 0, 1, 1], {0: dict(pairs_examined=4, pair_duplicates=3, pair_optical_duplicates=2)}),
    ("two_opticals_without_keeper", H_ONE_LIB,
     pair(nm(1, 9000, 9000, b"K"), rg=b"a") + pair(nm(1, 100, 100, b"A"), b"5", b"a") + pair(nm(1, 105, 100, b"B"), b"5", b"a"), 10, 0,
     [0, 1, 1], [0, 0, 1], {0: dict(pairs_examined=3, pair_duplicates=2, pair_optical_duplicates=1)}),
    ("group_of_four", H_ONE_LIB,
     pair(nm(1, 100, 100, b"K"), rg=b"a") + pair(nm(1, 104, 104, b"A"), b"5", b"a") + pair(nm(1, 500, 100, b"B"), b"5", b"a") +
     pair(nm(1, 500, 110, b"C"), b"5", b"a"), 10, 0,
     [0, 1, 1, 1], [0, 1, 0, 1], {0: dict(pairs_examined=4, pair_duplicates=3, pair_optical_duplicates=2)}),
    ("group_of_five", H_ONE_LIB,
     pair(nm(1, 100, 100, b"K"), rg=b"a") + pair(nm(1, 105, 100, b"A"), b"5", b"a") + pair(nm(1, 5000, 5000, b"B"), b"5", b"a") +
     pair(nm(1, 5005, 5000, b"C"), b"5", b"a") + pair(nm(1, 9000, 9000, b"E"), b"5", b"a"), 10, 0,
     [0, 1, 1, 1, 1], [0, 1, 0, 1, 0], {0: dict(pairs_examined=5, pair_duplicates=4, pair_optical_duplicates=2)}),
    ("other_tile", H_ONE_LIB, pair(nm(1, 100, 100, b"A"), rg=b"a") + pair(nm(2, 100, 100, b"B"), b"5", b"a"), 10, 0,
     [0, 1], [0, 0], {0: dict(pairs_examined=2, pair_duplicates=1)}),
    ("other_read_group_same_library", H_ONE_LIB, pair(nm(1, 100, 100, b"A"), rg=b"a") + pair(nm(1, 100, 100, b"B"), b"5", b"b"), 10, 0,
     [0, 1], [0, 0], {0: dict(pairs_examined=2, pair_duplicates=1)}),
    ("two_libraries", H_TWO_LIBS, pair(nm(1, 100, 100, b"A"), rg=b"a") + pair(nm(1, 100, 100, b"B"), b"5", b"c"), 10, 0,
     [0, 0], [0, 0], {0: PE, 1: PE}),
    ("none_against_none", H_ONE_LIB, pair(nm(1, 100, 100, b"A")) + pair(nm(1, 100, 100, b"B"), b"5", b"zz"), 10, 0,
     [0, 1], [0, 1], {1: dict(pairs_examined=2, pair_duplicates=1, pair_optical_duplicates=1)}),
    ("no_table", None, pair(nm(1, 100, 100, b"A"), rg=b"a") + pair(nm(1, 100, 100, b"B"), b"5", b"b"), 10, 0,
     [0, 1], [0, 1], {0: dict(pairs_examined=2, pair_duplicates=1, pair_optical_duplicates=1)}),
    ("member_without_location", H_ONE_LIB, pair(nm(1, 100, 100, b"A"), rg=b"a") + pair(b"plain", b"5", b"a") +
     pair(nm(1, 100, 100, b"B"), b"5", b"a"), 10, 0,
     [0, 1, 1], [0, 0, 1], {0: dict(pairs_examined=3, pair_duplicates=2, pair_optical_duplicates=1)}),
    ("group_over_max_set", H_ONE_LIB, pair(nm(1, 1, 1, b"A"), rg=b"a") + pair(nm(1, 1, 1, b"B"), b"5", b"a") +
     pair(nm(1, 1, 1, b"C"), b"5", b"a") + pair(nm(1, 1, 1, b"E"), b"5", b"a"), 10, 3,
     [0, 1, 1, 1], [0, 0, 0, 0], {0: dict(pairs_examined=4, pair_duplicates=3)}),
    ("group_of_max_set", H_ONE_LIB, pair(nm(1, 1, 1, b"A"), rg=b"a") + pair(nm(1, 1, 1, b"B"), b"5", b"a") +
     pair(nm(1, 1, 1, b"C"), b"5", b"a"), 10, 3,
     [0, 1, 1], [0, 1, 1], {0: dict(pairs_examined=3, pair_duplicates=2, pair_optical_duplicates=2)}),
    ("fr_and_rf_apart", H_ONE_LIB,
     [with_aux(rec(nm(1, 5, 5, b"A"), P1, 300), rgz(b"a")), with_aux(rec(nm(1, 5, 5, b"A"), P2 | R, 500), rgz(b"a")),
      with_aux(rec(nm(1, 5, 5, b"B"), P1 | R, 251), rgz(b"a")), with_aux(rec(nm(1, 5, 5, b"B"), P2, 549), rgz(b"a"))], 10, 0,
     [0, 0], [0, 0], {0: dict(pairs_examined=2)}),
    ("fragments_never_optical", H_ONE_LIB, frag(nm(1, 5, 5, b"A"), rg=b"a") + frag(nm(1, 5, 5, b"B"), b"5", b"a"), 10, 0,
     [0, 1], [0, 0], {0: dict(unpaired_examined=2, unpaired_duplicates=1)}),
    ("fragments_of_two_libraries", H_TWO_LIBS, frag(nm(1, 5, 5, b"A"), rg=b"a") + frag(nm(1, 5, 5, b"B"), b"5", b"c") +
     pair(nm(1, 5, 5, b"P"), rg=b"c", at=(300, 400)), 10, 0,             # a pair's end marks the fragments of its own library only
     [0, 1, 0], [0, 0, 0], {0: dict(unpaired_examined=1), 1: dict(unpaired_examined=1, unpaired_duplicates=1, pairs_examined=1)}),
    ("big_coordinates", H_ONE_LIB, pair(nm(-5, -2147483648, 2147483647, b"A"), rg=b"a") +
     pair(nm(-5, 2147483647, 2147483647, b"B"), b"5", b"a") + pair(nm(-5, -2147483648, 2147483640, b"C"), b"5", b"a"), 10, 0,
     [0, 1, 1], [0, 0, 1], {0: dict(pairs_examined=3, pair_duplicates=2, pair_optical_duplicates=1)}),
    ("records_of_every_kind", H_TWO_LIBS,
     frag(b"f", rg=b"a") + [with_aux(rec(b"f2", 0x4, -1, b"*", ref=b"*"), rgz(b"c"))] +
     [with_aux(rec(b"s", P1 | 0x8, 1500, qual=b"5"), rgz(b"c")), with_aux(rec(b"s", P1 | 0x8 | 0x800, 3000, b"30H20M", b"5", ref=b"c1"), b""),
      with_aux(rec(b"s", P1 | 0x8 | 0x100, 4000, b"50M", b"5"), b""), with_aux(rec(b"s", P1 | 0x100 | 0x4, 4000, b"50M", b"5"), b""),
      with_aux(rec(b"s", P2 | 0x4, 1500, b"*"), b"")], 10, 0,
     [0, 0, 0], [0, 0, 0], {0: dict(unpaired_examined=1), 1: dict(unpaired_examined=1, secondary_or_supplementary=2, unmapped=3)}),
    ("line_of_300", H_ONE_LIB, chain(300, 2), 2, 0, [0] + [1] * 299, [0] + [1] * 299,
     {0: dict(pairs_examined=300, pair_duplicates=299, pair_optical_duplicates=299)}),
    ("line_of_300_broken", H_ONE_LIB, chain(300, 2, broken=range(49, 300, 50)), 2, 0, [0] + [1] * 299,
     [int(i % 50 != 0) for i in range(300)], {0: dict(pairs_examined=300, pair_duplicates=299, pair_optical_duplicates=294)}),
]


def want_rows(n_lib: int, counts: dict) -> list:
    """the rows of a case: its hand-written counts, zeros elsewhere, rule 13's two derived values from them"""
    return [markdup.finish_row(dict(dict.fromkeys(markdup.LIB_COUNTS, 0), **counts.get(k, {}))) for k in range(n_lib)]


def tmpl_flags(records: bytes, rt) -> list:
    """0x400 per template, and that all records of a template agree"""
    out = {}
    for f, t in zip(flags(records), rt):
        assert out.setdefault(t, f & D) == f & D
    return [int(out[t] != 0) for t in sorted(out)]


@pytest.mark.parametrize("case", OPTICAL, ids=[c[0] for c in OPTICAL])
def test_rules_11_to_13(case):
    _, text, recs, d, max_set, dup, optical, counts = case
    table = markdup.groups(text) if text is not None else None
    n_lib = table.n_lib if table else 1
    n_t, es, rt, locs, _ = markdup.ends2(recs, table)
    got_dup, got_opt, rows = markdup.decide2(es, locs, n_t, n_lib, d, max_set or markdup.MAX_SET)
    assert ([int(x) for x in got_dup], [int(x) for x in got_opt]) == (dup, optical)
    want = want_rows(n_lib, counts)
    assert rows == [dict(r, secondary_or_supplementary=0, unmapped=0) for r in want]
    (out,), total, rows2 = markdup.mark2([b"".join(recs)], text, d, max_set or markdup.MAX_SET)
    assert rows2 == want and tmpl_flags(out, rt) == dup
    assert [f & ~D for f in flags(out)] == [f & ~D for f in flags(b"".join(recs))]
    for k in ("unpaired_examined", "pairs_examined", "unpaired_duplicates", "pair_duplicates"):
        assert total[k] == sum(r[k] for r in want)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_one_library_is_rules_1_to_8(case):
    _, recs, _, counts = case
    (a,), ca = markdup.mark([b"".join(recs)])
    (b,), cb, rows = markdup.mark2([b"".join(recs)])
    assert a == b and ca == cb and len(rows) == 1
    assert {k: rows[0][k] for k in counts if k in rows[0]} == {k: counts[k] for k in counts if k in rows[0]}


# ---- rule 14 ----

SIZES = [((1000, 900), 4660), ((10, 9), 46), ((2, 1), 1), ((500, 250), 313), ((1000000, 999999), 499999999999), ((3, 3), None),
         ((0, 0), None), ((5, 6), None), ((-1, -2), None), ((5, 0), None)]


@pytest.mark.parametrize("case", SIZES, ids=[str(c[0]) for c in SIZES])
def test_estimate_library_size(case):
    assert markdup.estimate_library_size(*case[0]) == case[1]


# ---- rule 15 ----

METRICS_ROWS = [dict(unpaired_examined=7, pairs_examined=1000, secondary_or_supplementary=3, unmapped=11, unpaired_duplicates=2,
                     pair_duplicates=100, pair_optical_duplicates=0),
                dict(unpaired_examined=0, pairs_examined=0, secondary_or_supplementary=0, unmapped=0, unpaired_duplicates=0,
                     pair_duplicates=0, pair_optical_duplicates=0),
                dict(unpaired_examined=3, pairs_examined=0, secondary_or_supplementary=0, unmapped=5, unpaired_duplicates=1,
                     pair_duplicates=0, pair_optical_duplicates=0)]
METRICS_TEXT = ("## htsjdk.samtools.metrics.StringHeader\n"
                "# bwams markdup lane1 lane2\n"
                "## METRICS CLASS\tpicard.sam.DuplicationMetrics\n"
                "LIBRARY\tUNPAIRED_READS_EXAMINED\tREAD_PAIRS_EXAMINED\tSECONDARY_OR_SUPPLEMENTARY_RDS\tUNMAPPED_READS\t"
                "UNPAIRED_READ_DUPLICATES\tREAD_PAIR_DUPLICATES\tREAD_PAIR_OPTICAL_DUPLICATES\tPERCENT_DUPLICATION\t"
                "ESTIMATED_LIBRARY_SIZE\n"
                "L1\t7\t1000\t3\t11\t2\t100\t0\t0.100648\t4660\n"
                "Unknown Library\t3\t0\t0\t5\t1\t0\t0\t0.333333\t\n"
                "\n")


def test_metrics_text():
    rows = [markdup.finish_row(dict(r)) for r in METRICS_ROWS]
    assert rows[0]["estimated_library_size"] == 4660 and rows[1]["estimated_library_size"] == -1
    assert rows[0]["percent_duplication"] == 202 / 2007
    assert markdup.metrics_text(markdup.groups(H_TWO_LIBS), rows, "bwams markdup lane1 lane2") == METRICS_TEXT
    one = markdup.metrics_text(None, rows[2:], "")
    assert one.split("\n")[1] == "# " and one.split("\n")[4].startswith("Unknown Library\t3\t0\t")
