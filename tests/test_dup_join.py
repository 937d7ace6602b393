"""Duplicate marking with templates joined by name (rules J1-J9, include/bwams.h above bwams_dupjoin_open): bwams/markdup.py's
name_key, join and mark_joined against rule J1's vectors, the hand-written flags and counts of tests/test_markdup.py, and
markdup.mark over the same records in query-grouped order.  tests/test_gpu_dup_join.py runs bwams_dupjoin_t against these."""
import pytest

from bwams import bam, markdup
from dup_join_cases import VECTORS, by_record, equivalence_input, key_names
from test_markdup import CASES, D, P1, P2, R, flags, rec
from test_markdup_metrics import H_TWO_LIBS, rgz, with_aux


def test_name_key():
    for name, want in VECTORS.items():
        assert markdup.name_key(name) == want, name
    names = key_names()
    assert sorted({len(n) for n in names[:8]}) == [0, 1, 7, 8, 9, 16, 17, 254]
    keys = [markdup.name_key(n) for n in names]
    assert len(set(keys)) == len(names)                       # the last-byte pair, the prefix pair and every length: all apart
    assert all(0 <= k < 1 << 64 for key in keys for k in key)
    assert len({k0 for k0, _ in keys}) == len(names) and len({k1 for _, k1 in keys}) == len(names)
    assert names[-3][:-1] == names[-4][:-1] and names[-2].startswith(names[-1])
    short = [bytes([a, b]) for a in range(256) for b in range(0, 256, 17)]                     # one length <= 8: one bijective step
    assert len({markdup.name_key(n)[0] for n in short}) == len(short)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_cases(case):
    _, recs, want, counts = case
    (out,), got, rows = markdup.mark_joined([b"".join(recs)])
    assert [f & D for f in flags(out)] == want
    assert [f & ~D for f in flags(out)] == [f & ~D for f in flags(b"".join(recs))]
    assert {k: got[k] for k in counts} == counts
    per_record = markdup.mark_joined([r for r in recs])[0]                                     # an add per record: the same marks
    assert b"".join(per_record) == out


def test_equivalence_with_query_grouped_order():
    templates, sorted_recs = equivalence_input()
    grouped = [r for t in templates for r in t]
    assert len(templates) >= 1000 and len(grouped) >= 1800
    assert sorted(grouped) == sorted(sorted_recs) and grouped != sorted_recs
    names = [r[36:36 + r[12]] for r in sorted_recs]
    assert any(names.index(n) + 1 < len(names) - 1 - names[::-1].index(n) for n in set(names))          # a template's records apart
    (a,), ca = markdup.mark([b"".join(grouped)])
    (b,), cb, _ = markdup.mark_joined([b"".join(sorted_recs)])
    A, B = by_record(a), by_record(b)
    assert set(A) == set(B) and sum(A[k] != B[k] for k in A) == 0                              # every record: the same bytes
    assert {k: cb[k] for k in ca} == ca
    assert ca["pair_duplicates"] > 100 and ca["unpaired_duplicates"] > 100
    pieces = [sorted_recs[:700], sorted_recs[700:701], [], sorted_recs[701:]]                  # the adds' cut changes nothing
    out, cc, _ = markdup.mark_joined([b"".join(p) for p in pieces])
    assert b"".join(out) == b and cc == cb and [len(bam.split_records(o)) for o in out] == [700, 1, 0, len(sorted_recs) - 701]


def test_ties_go_to_the_earlier_template():
    a, b = rec(b"ta", 0, 400), rec(b"tb", 0, 400)
    filler = [rec(b"f%d" % k, 0, 1000 + 10 * k) for k in range(3)]
    for first, second in ((a, b), (b, a)):
        (out,), _, _ = markdup.mark_joined([b"".join([first] + filler + [second])])
        assert [f & D for f in flags(out)] == [0, 0, 0, 0, D]                                   # J5: the kept one flips with the order


def test_refusals():
    far = [rec(b"n%d" % k, 0, 10 * k) for k in range(1000)]
    with pytest.raises(markdup.MarkdupRefusal) as e:                                            # J3: 1000 records apart
        markdup.join([b"".join([rec(b"twice", 0, 5)] + far + [rec(b"twice", 0, 20000)])])
    assert (e.value.record, e.value.reason) == (1001, 0)
    assert markdup.mark([b"".join([rec(b"twice", 0, 5)] + far + [rec(b"twice", 0, 20000)])])[1]["templates"] == 1002     # rule 1: two
    table = markdup.groups(H_TWO_LIBS)
    bad = b"RGZabc"                                                                             # a Z value without its NUL
    recs = [with_aux(rec(b"t", P1, 300), rgz(b"a")), with_aux(rec(b"t", P2 | R, 500), rgz(b"a")),
            with_aux(rec(b"t", P1 | 0x100, 900), bad)]                                          # rule 9 alone never walks a secondary
    assert markdup.ends2(recs, table)[0] == 1
    with pytest.raises(markdup.MarkdupRefusal) as e:
        markdup.join([b"".join(recs[:2]), b"".join(recs[2:])], table)
    assert (e.value.record, e.value.reason) == (2, markdup.AUX)
    assert markdup.join([b"".join(recs)], None)[0] == 1                                         # without a table nothing is walked
    several = [rec(b"ok", 0, 10), rec(b"m", 0, 20), rec(b"d", 0, 10), rec(b"x", 0, 50), rec(b"d", 0, 10), rec(b"m", 0x1 | 0x40, 20)]
    with pytest.raises(markdup.MarkdupRefusal) as e:                                            # d faults at 4, m at 5
        markdup.join([b"".join(several)])
    assert (e.value.record, e.value.reason) == (4, 0)
    with pytest.raises(markdup.MarkdupRefusal) as e:
        markdup.join([b"".join(several[:4]), b"".join(reversed(several[4:]))])                  # m now faults at 4 (mixed), d at 5
    assert (e.value.record, e.value.reason) == (4, 2)
