"""Collating by read name, the restatement (bwams/collate.py) against rules C1-C5 of include/bwams.h stated independently: hand
cases with their outputs written out in collate_cases.py, and on the equivalence input of the name join the properties the rules
imply, found here by grouping the names directly.  tests/test_gpu_collate.py runs the same cases through bwams_collate_t."""
import pytest

from bwams import collate
from collate_cases import CASES, REFUSALS, cuts, flag_of, joined, kept
from dup_join_cases import equivalence_input, names_of


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_cases(case):
    _, adds, want, orphans = case
    for form in (adds, joined(adds)):                        # lists of records, and byte strings
        got, left = collate.collate(form)
        assert got == want and left == orphans


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_name_the_ordinal_and_leave_the_state(case):
    _, adds, bad_add, ordinal, reason = case
    c = collate.Collate()
    for a in adds[:bad_add]:
        c.add(a)
    before = (dict(c.pending), c.records, c.skipped, c.pairs, c.singles, c.adds, c.bytes_pooled)
    with pytest.raises(collate.Refused) as e:
        c.add(adds[bad_add])
    assert (e.value.ordinal, e.value.reason) == (ordinal, reason) and f"record {ordinal}: " in str(e.value)
    assert (dict(c.pending), c.records, c.skipped, c.pairs, c.singles, c.adds, c.bytes_pooled) == before
    with pytest.raises(collate.Refused):
        collate.collate(adds)


@pytest.fixture(scope="module")
def sorted_recs():
    return equivalence_input()[1]


def direct_pairs(recs) -> set:
    """C3 without a walk: names are unique to a template here, so a name's kept paired records are its first and its last"""
    by_name = {}
    for r, nm in zip(recs, names_of(recs)):
        if kept(r) and flag_of(r) & 1:
            by_name.setdefault(nm, []).append(r)
    out = set()
    for v in by_name.values():
        assert len(v) <= 2
        if len(v) == 2:
            first, last = (v[0], v[1]) if flag_of(v[0]) & 0x40 else (v[1], v[0])
            assert flag_of(first) & 0xC0 == 0x40 and flag_of(last) & 0xC0 == 0x80
            out.add((first, last))
    return out


def test_equivalence_input_under_cuts(sorted_recs):
    recs = sorted_recs
    want_pairs = direct_pairs(recs)
    assert len(want_pairs) > 100 and any(not kept(r) for r in recs) and any(kept(r) and not flag_of(r) & 1 for r in recs)
    ordinal = {r: k for k, r in enumerate(recs)}             # the records are distinct
    assert len(ordinal) == len(recs)
    for how in ("one", "each", "thirds", "empty_middle"):
        adds = cuts(recs, how)
        outs, orphans = collate.collate(adds)
        assert len(outs) == len(adds)
        emitted = [r for pairs, singles in outs for p in pairs for r in p] + [r for _, singles in outs for r in singles] + orphans
        assert sorted(emitted) == sorted(r for r in recs if kept(r))                            # a permutation of the kept records
        got_pairs = [p for pairs, _ in outs for p in pairs]
        for first, last in got_pairs:                                                           # (first, last) of one name
            assert names_of([first]) == names_of([last])
            assert flag_of(first) & 0xC1 == 0x41 and flag_of(last) & 0xC1 == 0x81
        assert set(got_pairs) == want_pairs and len(got_pairs) == len(want_pairs)               # whatever the cut
        base = 0
        for a, (pairs, singles) in zip(adds, outs):
            done = [max(ordinal[f], ordinal[l]) for f, l in pairs]
            assert done == sorted(done) and all(base <= d < base + len(a) for d in done)        # by completing ordinal, in this add
            assert singles == [r for r in a if kept(r) and not flag_of(r) & 1]                  # the add's singles in order
            base += len(a)
        assert [ordinal[r] for r in orphans] == sorted(ordinal[r] for r in orphans)
        assert all(flag_of(r) & 1 for r in orphans)


def test_counters(sorted_recs):
    c = collate.Collate()
    recs = sorted_recs[:257]
    for a in cuts(recs, "thirds"):
        c.add(a)
    n_orphans = len(c.finish())
    n_kept = sum(kept(r) for r in recs)
    assert c.records == len(recs) and c.skipped == len(recs) - n_kept
    assert 2 * c.pairs + c.singles + n_orphans == n_kept and c.orphans == n_orphans and c.adds == 3
