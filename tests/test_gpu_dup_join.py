"""Duplicate marking with templates joined by name on the GPU (csrc/dup_join.hip, bwams_dupjoin_t): every comparison is exact,
against bwams/markdup.py's join / mark_joined (rules J1-J9, include/bwams.h above bwams_dupjoin_open), and for the equivalence
input also against the query-grouped path on the GPU (bwams_bam_upload + bwams_bam_markdup2)."""

import numpy as np
import pytest

import bam_query_cases as Q
from bwams import bai, bam, capi, depth, markdup, simulate
from dup_join_cases import by_record, equivalence_input, key_names, names_of
from test_markdup import CASES, D, P1, P2, R, flags, rec
from test_markdup_metrics import nm, pair, rgz, with_aux

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -3, -4, -6
H_LIBS = "@RG\tID:a\tLB:L1\n@RG\tID:c\tLB:L2\n@RG\tID:n\tSM:s\n"      # two read groups of different LB and one without


def dicts(rows, dtype) -> list:
    return [{k: int(x[k]) for k in dtype.names} for x in rows]


def check_join(j, adds, text=None, d=0, max_set=0):
    """adds through add_records / finish / fetch / apply_records on handle j (reset first): all equal to the restatement; returns
    (ends, rec_tmpl, dup, optical, rows, the marked adds, the stats)"""
    table = markdup.groups(text) if text is not None else None
    n_lib = table.n_lib if table else 1
    j.reset()
    assert [j.add_records(a) for a in adds] == [len(bam.split_records(a)) for a in adds]
    st, rows = j.finish()
    ends, locs, rt, dup, optical = j.fetch()
    wn, wends, wrt, wlocs, _ = markdup.join(adds, table)
    assert dicts(ends, capi.DUP_END_DTYPE) == wends and dicts(locs, capi.DUP_LOC_DTYPE) == wlocs          # field by field
    assert rt.tolist() == wrt and len(dup) == wn
    wdup, wopt, _ = markdup.decide2(wends, wlocs, wn, n_lib, d, max_set or markdup.MAX_SET)
    assert dup.tolist() == [int(x) for x in wdup] and optical.tolist() == [int(x) for x in wopt]
    want, counts, wrows = markdup.mark_joined(adds, text, d, max_set or markdup.MAX_SET)
    assert st.counts() == {k: counts[k] for k in st.counts()}
    assert capi.lib_rows(rows) == wrows
    got = []
    for a, w in zip(adds, want):
        out, n = j.apply_records(a)
        assert out == w and n == sum(bool(f & D) for f in flags(out))
        got.append(out)
    i = j.info()
    assert (i["records"], i["templates"], i["ends"], i["adds"], i["applied"], i["state"]) == (len(wrt), wn, len(wends), len(adds), len(adds), 2)
    return ends, rt, dup, optical, rows, got, st


@pytest.fixture(scope="module")
def join():
    j = capi.DupJoin()
    yield j
    j.close()


@pytest.fixture(scope="module")
def equivalence():
    templates, sorted_recs = equivalence_input()
    (want,), counts, rows = markdup.mark_joined([b"".join(sorted_recs)])
    return templates, sorted_recs, want, counts, rows


def test_hand_cases_and_key(join):
    for name, recs, want, counts in CASES:
        data = b"".join(recs)
        _, _, _, _, _, (out,), st = check_join(join, [data])
        assert [f & D for f in flags(out)] == want, name
        assert [f & ~D for f in flags(out)] == [f & ~D for f in flags(data)], name                # every bit but 0x400 unchanged
        assert len(out) == len(data) and [r[:18] + r[20:] for r in bam.split_records(out)] == [r[:18] + r[20:] for r in recs], name
        assert {k: st.counts()[k] for k in counts} == counts, name
    for n in key_names():
        assert capi.dupjoin_key(n) == markdup.name_key(n), n
    with pytest.raises(capi.BwamsError) as e:
        capi.dupjoin_key(b"x" * 255)
    assert e.value.code == ERR_ARG


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_shapes(join, equivalence, n):
    """a wave of the entry kernel, one lane more or less, a second workgroup, nothing at all; the adds' cut changes nothing"""
    recs = equivalence[1][:n]
    one = check_join(join, [b"".join(recs)])
    each = check_join(join, [r for r in recs])
    c0, c1 = n // 5, (2 * n) // 3
    uneven = check_join(join, [b"".join(recs[:c0]), b"".join(recs[c0:c1]), b"".join(recs[c1:])])
    for other in (each, uneven):
        for a, b in zip(one[:5], other[:5]):
            assert a.tolist() == b.tolist()
        assert b"".join(other[5]) == b"".join(one[5])


def test_empty_add_in_the_middle(join, equivalence):
    recs = equivalence[1][:100]
    whole = check_join(join, [b"".join(recs)])
    parts = check_join(join, [b"".join(recs[:40]), b"", b"".join(recs[40:])])
    assert b"".join(parts[5]) == whole[5][0] and parts[1].tolist() == whole[1].tolist()


def _file(tmp_path, records: bytes) -> str:
    p = tmp_path / "sorted.bam"
    p.write_bytes(Q.bam_file(records, 300))
    return str(p)


def test_file_mates_across_pieces(tmp_path, equivalence):
    templates, sorted_recs, want, counts, wrows = equivalence
    records = b"".join(sorted_recs)
    assert len(records) >= 350000
    f = capi.BamFile(_file(tmp_path, records), piece_bytes=65536)
    j = capi.DupJoin()
    ix = capi.Index.build(simulate.make_genome(3000, seed=3, repeat_frac=0.0), 0)
    b = capi.Batch(ix, 4000, 4000 * 160)
    try:
        f.query()
        n_piece = []
        for p in f.pieces():
            n_piece.append(j.add_file(p))
        assert f.info()["pieces"] > 1 and sum(n_piece) == len(sorted_recs)
        piece_of = np.repeat(np.arange(len(n_piece)), n_piece)                                  # by piece record counts
        names = names_of(sorted_recs)
        spread = {}
        for nme, pc in zip(names, piece_of):
            spread.setdefault(nme, set()).add(int(pc))
        assert any(len(v) > 1 for v in spread.values())                                         # a template's records in two pieces
        st, rows = j.finish()
        assert st.counts() == {k: counts[k] for k in st.counts()} and capi.lib_rows(rows) == wrows
        f.query()
        got, marked = [], 0
        for p in f.pieces():
            marked += j.apply_file(p)
            got.append(p.fetch()[0])
        assert b"".join(got) == want and marked == counts["records_marked"]
        assert [len(bam.split_records(g)) for g in got] == n_piece
        # the existing path as a second yardstick: the query-grouped order through the batch
        grouped = b"".join(r for t in templates for r in t)
        assert b.bam_upload(grouped) == len(sorted_recs)
        b.bam_markdup2()
        A, B = by_record(b.bam_fetch()[0]), by_record(b"".join(got))
        assert set(A) == set(B) and all(A[k] == B[k] for k in A)
    finally:
        b.close()
        ix.close()
        j.close()
        f.close()


def test_writing_it(tmp_path, equivalence):
    _, sorted_recs, want, counts, _ = equivalence
    records = b"".join(sorted_recs)
    f = capi.BamFile(_file(tmp_path, records), piece_bytes=65536)
    j = capi.DupJoin()
    out_path = str(tmp_path / "marked.bam")
    try:
        assert f.header_block() == bam.header_block(Q.HEADER_TEXT, Q.NAMES, Q.LENS)
        f.query()
        for p in f.pieces():
            j.add_file(p)
        j.finish()
        s = capi.Sorter(out_path, 0, f.header_block(), bai=True)
        f.query()
        seen = b""
        for k, p in enumerate(f.pieces()):
            j.apply_file(p)
            recs, coords = p.fetch()
            if k == 1:                                                                          # a consumer on the piece sees the marks
                d = capi.Depth(Q.LENS)
                w = depth.Depth(Q.LENS)
                n_counted = w.add(recs)
                assert d.add_file(p) == n_counted < len(bam.split_records(recs))                 # 0x400 is in the default exclude
                assert np.array_equal(d.finish().fetch(0, 0, 400000), w.finish().depth[0][:400000])
                d.close()
            s.put(k, recs, coords)
            seen += recs
        s.close()
        assert seen == want
    finally:
        j.close()
        f.close()
    g = capi.BamFile(out_path)
    try:
        back, _ = g.read()
        assert back == want
    finally:
        g.close()
    with open(out_path, "rb") as fh, open(out_path + ".bai", "rb") as ih:
        assert ih.read() == bai.build(fh.read())


def test_libraries_and_optical():
    g = capi.DupGroups(H_LIBS)
    table = markdup.groups(H_LIBS)
    j = capi.DupJoin(g, distance=10)
    try:
        recs = []
        recs += pair(nm(1, 5000, 5000, b"la"), b"I", b"a") + pair(nm(1, 9000, 9000, b"lc"), b"5", b"c")      # one place, two libraries
        recs += pair(nm(2, 100, 100, b"ln"), b"5", b"n") + pair(nm(2, 900, 900, b"lu"), b"0", None)           # no LB, no RG: one library
        # the RG only on the primaries, the supplementary record (no RG) first in the file: J4's first primary
        sup = [rec(nm(3, 1, 1, b"sp"), P1 | 0x800, 10, b"30H20M", b"5")] + pair(nm(3, 1, 1, b"sp"), b"5", b"a", at=(1300, 1500))
        recs += sup + pair(nm(3, 700, 700, b"sq"), b"I", b"a", at=(1300, 1500))
        # an optical cluster of three, the kept pair outside it
        recs += pair(nm(7, 9000, 9000, b"ok"), b"I", b"c", at=(2300, 2500))
        recs += [r for k in range(3) for r in pair(nm(7, 100 + 8 * k, 100, b"o%d" % k), b"5", b"c", at=(2300, 2500))]
        data = bam.coord_sort(b"".join(recs))
        ends, rt, dup, optical, rows, (out,), _ = check_join(j, [data], H_LIBS, 10)
        name_t = dict(zip(names_of(data), rt.tolist()))
        is_dup = lambda tag: bool(dup[next(t for n, t in name_t.items() if n.startswith(tag + b":"))])     # noqa: E731
        assert not is_dup(b"la") and not is_dup(b"lc")                                          # equal places, two libraries
        assert not is_dup(b"ln") and is_dup(b"lu")                                              # both "Unknown Library"
        assert is_dup(b"sp") and not is_dup(b"sq")                                              # library L1 by its first primary
        assert names_of(data)[0].startswith(b"sp:") and bam.split_records(data)[0][18 + 1] & 0x08     # the supplementary record leads
        assert optical.sum() == 2 and [is_dup(b"o%d" % k) for k in range(3)] == [True] * 3 and not is_dup(b"ok")
        wrows = markdup.mark_joined([data], H_LIBS, 10)[2]
        assert capi.dup_metrics_text(g, rows, "joined") == markdup.metrics_text(table, wrows, "joined")
        assert [r["pair_optical_duplicates"] for r in wrows] == [0, 2, 0]
    finally:
        j.close()
        g.close()


def _refused(code, text, fn, *args):
    with pytest.raises(capi.BwamsError) as e:
        fn(*args)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_refusals_and_states(tmp_path, equivalence):
    L = capi.lib()
    g = capi.DupGroups(H_LIBS)
    j, jg = capi.DupJoin(), capi.DupJoin(g)
    try:
        # J3: two primaries of one segment 1000 records apart
        far = b"".join(rec(b"n%d" % k, 0, 10 * k) for k in range(1000))
        j.add_records(rec(b"twice", 0, 5) + far + rec(b"twice", 0, 20000))
        _refused(ERR_UNSUPPORTED, "bwams_dupjoin_finish: record 1001: " + markdup.REASONS[0], j.finish)
        for fn, args in ((j.add_records, (far,)), (j.finish, ()), (j.fetch, ()), (j.apply_records, (far,))):     # only _reset or _close
            _refused(ERR_ARG, "only bwams_dupjoin_reset and _close remain", fn, *args)
        j.reset()
        several = [rec(b"ok", 0, 10), rec(b"m", 0, 20), rec(b"d", 0, 10), rec(b"x", 0, 50), rec(b"d", 0, 10), rec(b"m", 0x1 | 0x40, 20)]
        j.add_records(b"".join(several))
        _refused(ERR_UNSUPPORTED, "bwams_dupjoin_finish: record 4: " + markdup.REASONS[0], j.finish)         # the smallest ordinal
        j.reset()
        # J4: a secondary record that rule 9 alone would never walk
        good = [with_aux(rec(b"t", P1, 300), rgz(b"a")), with_aux(rec(b"t", P2 | R, 500), rgz(b"a"))]
        bad = with_aux(rec(b"t", P1 | 0x100, 900), b"RGZabc")
        assert jg.add_records(good[0]) == 1
        _refused(ERR_UNSUPPORTED, "bwams_dupjoin_add_records: record 2: " + markdup.REASONS[markdup.AUX], jg.add_records, good[1] + bad)
        assert jg.info()["records"] == 1 and jg.info()["adds"] == 1
        assert jg.add_records(good[1]) == 1                                                     # as if the bad add had never come
        small = np.zeros(2, capi.DUP_LIB_STATS_DTYPE)
        assert L.bwams_dupjoin_finish(jg.h, None, capi._p(small), 2) == ERR_CAPACITY            # three libraries
        st, rows = jg.finish()
        assert st.counts() == {k: v for k, v in markdup.mark_joined(good, H_LIBS)[1].items() if k in st.counts()}
        assert jg.fetch()[2].tolist() == [0, 0]
        j.add_records(good[1] + bad)                                                            # without a table nothing is walked
        assert j.finish()[0].templates == 1
        j.reset()
        # J9
        recs = equivalence[1][:200]
        a, b2 = b"".join(recs[:120]), b"".join(recs[120:])
        _refused(ERR_ARG, "call bwams_dupjoin_finish first", j.fetch)
        _refused(ERR_ARG, "call bwams_dupjoin_finish first", j.apply_records, a)
        j.add_records(a)
        _refused(ERR_ARG, "call bwams_dupjoin_finish first", j.apply_records, a)
        j.add_records(b2)
        st, _ = j.finish()
        _refused(ERR_ARG, "bwams_dupjoin_reset starts another round", j.add_records, a)
        _refused(ERR_ARG, "bwams_dupjoin_reset starts another round", j.finish)
        # cap_* too small
        i = j.info()
        ends = np.zeros(i["ends"], capi.DUP_END_DTYPE)
        rt, dup = np.zeros(i["records"], np.uint32), np.zeros(i["templates"], np.uint8)
        for caps in ((i["ends"] - 1, i["records"], i["templates"]), (i["ends"], i["records"] - 1, i["templates"]),
                     (i["ends"], i["records"], i["templates"] - 1)):
            assert L.bwams_dupjoin_fetch(j.h, capi._p(ends), None, caps[0], capi._p(rt), caps[1], capi._p(dup), None, caps[2]) == ERR_CAPACITY
        assert L.bwams_dupjoin_fetch(j.h, None, None, 0, None, 0, None, None, 0) == 0           # any pointer NULL
        # J8: one record fewer; two names exchanged at the same count: nothing is written, and the right records still apply
        want = markdup.mark_joined([a, b2])[0]
        assert want[0] != a
        fewer = np.frombuffer(b"".join(recs[:119]), np.uint8).copy()
        swapped = recs[:120]
        swapped[3], swapped[77] = swapped[77], swapped[3]
        assert names_of(swapped) != names_of(recs[:120]) and sorted(names_of(swapped)) == sorted(names_of(recs[:120]))
        swapped = np.frombuffer(b"".join(swapped), np.uint8).copy()
        for buf in (fewer, swapped):
            before = buf.copy()
            assert L.bwams_dupjoin_apply_records(j.h, capi._p(buf), len(buf), None) == ERR_ARG
            assert L.bwams_last_error().decode().startswith("bwams_dupjoin_apply_records: apply 0")
            assert (buf == before).all()
        assert j.apply_records(a)[0] == want[0] and j.apply_records(b2)[0] == want[1]
        _refused(ERR_ARG, "every one of the 2 adds has been applied", j.apply_records, b2)      # an apply past the last add
        with pytest.raises(capi.BwamsError):                                                    # a device that is not there
            capi.DupJoin(device=1 << 20)
        # _reset and a second full round on the same handle
        j.reset()
        assert j.info()["records"] == 0 and j.info()["state"] == 0
        j.add_records(b2)
        assert j.finish()[0].counts() == {k: v for k, v in markdup.mark_joined([b2])[1].items() if k in st.counts()}
        assert j.apply_records(b2)[0] == markdup.mark_joined([b2])[0][0]
    finally:
        j.close()
        jg.close()
        g.close()
