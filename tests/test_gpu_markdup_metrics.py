"""Duplicate marking's rules 9-15 on the GPU (csrc/markdup.hip: bwams_bam_templates2 / _templates_fetch_loc, bwams_dup_decide2,
bwams_bam_markdup2), in the sorted BAM writer (bwams_sorter_set_markdup / _close3) and the host's metrics text, against
bwams/markdup.py's restatement and the hand-written expectations of tests/test_markdup_metrics.py."""
import ctypes as C
import gzip
import struct

import numpy as np
import pytest

from bwams import bai, bam, capi, markdup, simulate
from test_gpu_markdup import _fq, toy                                            # noqa: F401  (toy: the two-sequence index)
from test_markdup import CASES, D, P1, P2, R, flags, rec
from test_markdup_metrics import (GROUPS, GROUPS_REFUSED, H_NO_RG, H_ONE_LIB, H_TWO_LIBS, METRICS_ROWS, METRICS_TEXT, NAMES, OPTICAL,
                                  REFUSED, SIZES, WALKS, frag, pair, rgz, tmpl_flags, want_rows, with_aux)

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -3, -4, -6
COUNTS4 = ("unpaired_examined", "unpaired_duplicates", "pairs_examined", "pair_duplicates")


@pytest.fixture(scope="module")
def batch(toy):                                                                  # noqa: F811
    _, ix = toy
    b = capi.Batch(ix, 100, 100 * 160)
    yield b
    b.close()


def rows_of(lib_stats) -> list:
    return capi.lib_rows(lib_stats)


def loc_dicts(loc) -> list:
    return [{k: int(x[k]) for k in capi.DUP_LOC_DTYPE.names} for x in loc]


def end_dicts(ends) -> list:
    return [{k: int(e[k]) for k in capi.DUP_END_DTYPE.names} for e in ends]


def check_batch(b, recs, text, d, max_set=0):
    """records through bwams_bam_upload: templates2 + fetch_loc and decide2, then markdup2, all equal to the restatement; returns
    (dup, optical: per template, rows of markdup2, the restatement's rows, each record's template)"""
    data = b"".join(recs) if not isinstance(recs, bytes) else recs
    table = markdup.groups(text) if text is not None else None
    g = capi.DupGroups(text) if text is not None else None
    n_lib = table.n_lib if table else 1
    b.bam_upload(data)
    n_t, n_e = b.bam_templates2(g)
    ends, rt = b.bam_templates_fetch()
    loc = b.bam_templates_fetch_loc()
    wn, wends, wrt, wlocs, wtlib = markdup.ends2(data, table)
    assert (n_t, n_e, rt.tolist()) == (wn, len(wends), wrt)
    assert end_dicts(ends) == wends and loc_dicts(loc) == wlocs
    dup, optical, rows = capi.dup_decide2(0, ends, loc, n_t, n_lib, d, max_set)
    wdup, wopt, wrows = markdup.decide2(wends, wlocs, wn, n_lib, d, max_set or markdup.MAX_SET)
    assert dup.tolist() == [int(x) for x in wdup] and optical.tolist() == [int(x) for x in wopt]
    assert rows_of(rows) == wrows
    (want,), counts, wrows2 = markdup.mark2([data], text, d, max_set or markdup.MAX_SET)
    st, rows2 = b.bam_markdup2(g, d, max_set)
    out, _ = b.bam_fetch()
    assert out == want and rows_of(rows2) == wrows2
    assert st.counts() == {k: counts[k] for k in st.counts()}
    ss, un = b.bam_lib_record_counts(n_lib)
    assert ss.tolist() == [r["secondary_or_supplementary"] for r in wrows2] and un.tolist() == [r["unmapped"] for r in wrows2]
    if g:
        g.close()
    return dup.tolist(), optical.tolist(), rows_of(rows2), wrows2, rt.tolist()


def test_symbols_and_host_rules():
    """the groups table, rule 14 and rule 15 through the C-ABI"""
    for _, text, ids, rg_lib, libs in GROUPS:
        g = capi.DupGroups(text)
        assert (g.n_rg, g.n_lib, g.libraries) == (len(ids), len(libs), libs) and g.library(len(libs)) is None
        g.close()
    for _, text in GROUPS_REFUSED:
        with pytest.raises(capi.BwamsError) as e:
            capi.DupGroups(text)
        assert e.value.code == ERR_ARG
    for (n, c), want in SIZES:
        assert capi.dup_library_size(n, c) == want
    rows = np.zeros(3, capi.DUP_LIB_STATS_DTYPE)
    for k, r in enumerate(METRICS_ROWS):
        w = markdup.finish_row(dict(r))
        for f in capi.DUP_LIB_STATS_DTYPE.names:
            rows[k][f] = w[f]
    g = capi.DupGroups(H_TWO_LIBS)
    assert capi.dup_metrics_text(g, rows, "bwams markdup lane1 lane2") == METRICS_TEXT
    with pytest.raises(capi.BwamsError) as e:
        capi.dup_metrics_text(g, rows[:2], "")                                     # the table has three libraries
    assert e.value.code == ERR_ARG
    g.close()


@pytest.mark.parametrize("case", OPTICAL, ids=[c[0] for c in OPTICAL])
def test_hand_built_cases(batch, case):
    _, text, recs, d, max_set, dup, optical, counts = case
    got_dup, got_opt, rows, wrows, rt = check_batch(batch, recs, text, d, max_set)
    assert (got_dup, got_opt) == (dup, optical)
    assert rows == want_rows(len(rows), counts)
    out, _ = batch.bam_fetch()
    assert tmpl_flags(out, rt) == dup
    assert [f & ~D for f in flags(out)] == [f & ~D for f in flags(b"".join(recs))]     # nothing but 0x400 differs


def test_aux_walk(batch):
    L = capi.lib()
    ids = sorted({w for _, _, w in WALKS if isinstance(w, bytes)})
    text = "".join("@RG\tID:%s\tLB:lib%d\n" % (x.decode(), k % 2) for k, x in enumerate(ids))
    table = markdup.groups(text)
    g = capi.DupGroups(text)
    good = [(aux, w) for _, aux, w in WALKS if w is not REFUSED]
    recs = [with_aux(rec(b"t%d" % k, 0, 10 + 100 * k), aux) for k, (aux, _) in enumerate(good)]
    batch.bam_upload(b"".join(recs))
    batch.bam_templates2(g)
    loc = batch.bam_templates_fetch_loc()
    assert loc["rg"].tolist() == [table.ids.index(w) if w is not None else -1 for _, w in good]
    assert loc["lib"].tolist() == [table.lib_of(r) for r in loc["rg"].tolist()]
    assert loc_dicts(loc) == markdup.ends2(recs, table)[3]
    nt, ne = C.c_int64(0), C.c_int64(0)
    for name, aux, w in WALKS:
        if w is not REFUSED:
            continue
        batch.bam_upload(rec(b"ok", 0, 5) + with_aux(rec(b"n", 0, 10), aux))
        assert L.bwams_bam_templates2(batch.h, g.h, C.byref(nt), C.byref(ne)) == ERR_UNSUPPORTED, name
        assert L.bwams_last_error().decode() == "bwams_bam_templates: record 1: aux fields do not chain to the record's end", name
        assert L.bwams_bam_markdup2(batch.h, g.h, None, None, None, 0) == ERR_UNSUPPORTED, name
        assert batch.bam_templates2(None) == (2, 2), name                                     # no table: nothing is walked
        assert batch.bam_templates_fetch_loc()["rg"].tolist() == [-1, -1]
        assert batch.bam_markdup().templates == 2                                             # and the calls of rules 1-8 accept it
    bad = b"RGZabc"                                           # the record walked: the first primary, else the first record
    recs = [with_aux(rec(b"t", P1 | 0x800, 900, b"20M30H"), bad), with_aux(rec(b"t", P2 | R, 500), rgz(b"one")),
            with_aux(rec(b"t", P1, 300), rgz(b"a")), with_aux(rec(b"u", 0x100, 40), rgz(b"a")), with_aux(rec(b"u", 0x100, 50), bad)]
    check_batch(batch, recs, text, 0)
    batch.bam_upload(with_aux(rec(b"x", 0, 5), bad) + rec(b"a", 0, 5, ref=b"*"))       # rules 2-3 refuse first, also at a later record
    assert L.bwams_bam_templates2(batch.h, g.h, C.byref(nt), C.byref(ne)) == ERR_UNSUPPORTED
    assert L.bwams_last_error().decode().startswith("bwams_bam_templates: record 1: " + markdup.REASONS[3])
    g.close()


def test_names(batch):
    long7 = b"M" * (254 - len(b":1:FC:2:1101:77:88")) + b":1:FC:2:1101:77:88"
    long0 = b"q" * 254
    names = [n for n, _ in NAMES] + [long7, long0]
    assert len(long7) == 254 and markdup.location(long7) == (1101, 77, 88)
    recs = []
    for k, n in enumerate(names):                                                # no aux bytes, and an RG behind the longest names
        recs += frag(n, at=50 * k, rg=b"a" if len(n) == 254 else None)
    batch.bam_upload(b"".join(recs))
    g = capi.DupGroups(H_ONE_LIB)
    assert batch.bam_templates2(g) == (len(names), len(names))
    loc = batch.bam_templates_fetch_loc()
    want = [markdup.location(n) for n in names]
    assert [(int(x["tile"]), int(x["x"]), int(x["y"])) if x["has"] else None for x in loc] == want
    assert want[:len(NAMES)] == [w for _, w in NAMES]
    assert all((x["tile"], x["x"], x["y"]) == (0, 0, 0) for x in loc if not x["has"])
    assert loc["rg"].tolist() == [-1] * len(NAMES) + [0, 0]
    g.close()
    check_batch(batch, recs, H_ONE_LIB, 5)


def test_70_libraries(batch):
    text = "".join("@RG\tID:rg%d\tLB:lib%d\n" % (k, k) for k in range(70)) + "@RG\tID:nolb\n"
    recs = []
    for k in range(70):
        rg = b"rg%d" % k
        recs += pair(b"x:l:1:%d:5" % k, rg=rg) + frag(b"f%d" % k, rg=rg, at=900)
        if k % 3 == 0:
            recs += pair(b"y:l:1:%d:9" % k, b"5", rg)
        if k % 7 == 0:
            recs += frag(b"g%d" % k, b"5", rg, at=900) + [with_aux(rec(b"u%d" % k, 0x4, -1, b"*", ref=b"*"), rgz(rg))]
    recs += pair(b"x:l:1:0:5", rg=b"nolb") + pair(b"y:l:1:3:5", b"5", None)
    _, _, rows, wrows, _ = check_batch(batch, recs, text, 10)
    assert len(rows) == 71 and rows[0]["pair_optical_duplicates"] == 1 and rows[70]["pair_duplicates"] == 1
    assert sum(r["pair_duplicates"] for r in rows) == 24 + 1 and sum(r["unpaired_duplicates"] for r in rows) == 10
    assert sum(r["unmapped"] for r in rows) == 10


def test_one_library_with_a_table_and_empty_batch(batch):
    recs = pair(b"x:l:1:5:5", rg=b"z") + pair(b"y:l:1:6:5", b"5", b"other") + frag(b"f", at=300)
    _, optical, rows, _, _ = check_batch(batch, recs, H_NO_RG, 10)
    assert len(rows) == 1 and optical == [0, 1, 0] and rows[0]["unpaired_duplicates"] == 1
    for text in (None, H_TWO_LIBS):
        dup, optical, rows, wrows, _ = check_batch(batch, b"", text, 10)
        assert dup == [] and optical == [] and rows == wrows and all(r["estimated_library_size"] == -1 for r in rows)
        g = capi.DupGroups(text) if text else None
        assert capi.dup_metrics_text(g, batch.bam_markdup2(g, 10)[1], "none").count("\n") == 5       # no row


def test_legacy_equality(batch):
    for name, recs, want, counts in CASES:
        data = b"".join(recs)
        batch.bam_upload(data)
        st0 = batch.bam_markdup()
        out0, _ = batch.bam_fetch()
        for opt in (True, False):
            batch.bam_upload(data)
            st, rows = batch.bam_markdup2(None, 0, 0, opt=opt)
            assert batch.bam_fetch()[0] == out0 and st.counts() == st0.counts() == counts, name
            row = rows_of(rows)[0]
            assert {k: row[k] for k in COUNTS4} == {k: counts[k] for k in COUNTS4}, name
            assert row == markdup.mark2([data])[2][0], name
        n_t, n_e = batch.bam_templates()
        ends, _ = batch.bam_templates_fetch()
        dup0, dst0 = capi.dup_decide(0, ends, n_t)
        dup, optical, rows = capi.dup_decide2(0, ends, None, n_t, 1, 100, 0)
        assert dup.tolist() == dup0.tolist() and not optical.any(), name
        assert {k: rows_of(rows)[0][k] for k in COUNTS4} == {k: dst0.counts()[k] for k in COUNTS4}, name


def test_argument_errors(batch):
    _, text, recs, d, _, dup, optical, _ = OPTICAL[0]
    assert optical == [0, 1]
    g = capi.DupGroups(text)
    batch.bam_upload(b"".join(recs))
    n_t, _ = batch.bam_templates2(g)
    ends, _ = batch.bam_templates_fetch()
    loc = batch.bam_templates_fetch_loc()
    for field, value in (("lib", 2), ("lib", -1), ("has", 2)):
        bad = loc.copy()
        bad[field][1] = value
        with pytest.raises(capi.BwamsError) as e:
            capi.dup_decide2(0, ends, bad, n_t, 2, d)
        assert e.value.code == ERR_ARG and "bwams_dup_decide: end 1: loc.lib outside [0, n_lib)" in str(e.value)
    with pytest.raises(capi.BwamsError) as e:
        batch.bam_markdup2(g, d, cap_lib=1)
    assert e.value.code == ERR_CAPACITY
    got_dup, got_opt, rows = capi.dup_decide2(0, ends, loc, n_t, 2, d, opt=False)     # a NULL opt: optical detection off
    assert got_dup.tolist() == dup and not got_opt.any() and rows_of(rows)[0]["pair_optical_duplicates"] == 0
    st, rows = batch.bam_markdup2(g, d, opt=False)
    assert st.pair_duplicates == 1 and rows_of(rows)[0]["pair_optical_duplicates"] == 0
    assert rows_of(batch.bam_markdup2(g, d)[1])[0]["pair_optical_duplicates"] == 1
    batch.bam_upload(b"".join(recs))                                                  # fetch_loc wants templates2 on these records
    batch.bam_templates()
    with pytest.raises(capi.BwamsError) as e:
        batch.bam_templates_fetch_loc()
    assert e.value.code == ERR_ARG
    g.close()


# ---- a simulated batch: three read groups over two libraries, Illumina names, planted copies around d ----

HEADER_RG = "@RG\tID:lane1\tLB:libA\tSM:s\n@RG\tID:lane2\tLB:libA\tSM:s\n@RG\tID:lane3\tLB:libB\tSM:s\n"
DIST = 100


def _name(rng, lane, tile=None, x=None, y=None):
    return b"M:1:FC:%d:%d:%d:%d" % (lane, tile if tile is not None else 1101 + int(rng.integers(0, 3)),
                                    x if x is not None else int(rng.integers(1000, 20000)), y if y is not None else int(rng.integers(1000, 20000)))


def _near(rng, name):
    """another name on the same lane and tile whose x and y lie within about 2 d of name's: inside d, at d, or past it"""
    f = name.split(b":")
    off = lambda: int(rng.choice([0, 3, DIST - 1, DIST, DIST + 1, 2 * DIST])) * int(rng.choice([-1, 1]))      # noqa: E731
    dx, dy = off(), off()
    return b":".join(f[:5] + [b"%d" % (int(f[5]) + (dx or (3 if dy == 0 else 0))), b"%d" % (int(f[6]) + dy)])     # never the same name


def _chunks(g, seed):
    """three chunks (two of pairs, interleaved; one of single reads) as (FASTQ text, paired); copies are planted inside a chunk and,
    for chunk 1, of chunk 0's pairs; the lane in the name is the read group"""
    rng = np.random.default_rng(seed)
    out, first = [], None
    for c, n in enumerate((1500, 1500)):
        pr = simulate.make_read_pairs(g, n, seed=seed + c, damaged_frac=0.0, discordant_frac=0.0)
        e1, e2, nm, qs = [], [], [], []
        for i in range(n):
            a, b_ = pr[2 * i], pr[2 * i + 1]
            name = _name(rng, 1 + i % 3)
            e1.append(a); e2.append(b_); nm.append(name); qs.append(b"I")
            if i % 4 == 0:                                                        # a copy nearby, in the same read group
                e1.append(a); e2.append(b_); nm.append(_near(rng, name)); qs.append(b"5")
            if i % 10 == 0:                                                       # one in another read group: lane + 1
                f = _near(rng, name).split(b":")
                f[3] = b"%d" % (1 + (i + 1) % 3)
                e1.append(a); e2.append(b_); nm.append(b":".join(f)); qs.append(b"5")
            if i % 25 == 0:                                                       # three more on a line of steps below d: a chain
                f = name.split(b":")
                for k in range(1, 4):
                    e1.append(a); e2.append(b_); qs.append(b"5")
                    nm.append(b":".join(f[:5] + [b"%d" % (int(f[5]) + 60 * k), f[6]]))
        if c == 0:
            first = (e1[:40], e2[:40], nm[:40])
        else:                                                                     # copies of the other chunk's pairs
            for a, b_, name in zip(*first):
                e1.append(a); e2.append(b_); nm.append(_near(rng, name)); qs.append(b"5")
        t1, t2 = _fq(e1, nm, qs).split(b"\n"), _fq(e2, nm, qs).split(b"\n")
        out.append((b"".join(b"\n".join(t1[4 * i:4 * i + 4] + t2[4 * i:4 * i + 4]) + b"\n" for i in range(len(nm))), True))
    reads, _, _ = simulate.make_reads(g, 900, seed=seed + 7)
    rs, nm, qs = [], [], []
    for i, r in enumerate(reads):
        name = _name(rng, 1 + i % 3)
        rs.append(r); nm.append(name); qs.append(b"I")
        if i % 5 == 0:                                                        # every lane gets copies
            rs.append(r); nm.append(_near(rng, name)); qs.append(b"5")
    out.append((_fq(rs, nm, qs), False))
    return out


@pytest.fixture(scope="module")
def simulated(toy):                                                              # noqa: F811
    """the three chunks aligned, their records with RG:Z:lane<n> added by re-encoding; the restatement's result over them as one input"""
    g, ix = toy
    names = [b"chrA", b"chrB"]
    ref_id = {n: k for k, n in enumerate(names)}
    runs = []
    b = capi.Batch(ix, 6000, 6000 * 160)
    try:
        base = 0
        for text, paired in _chunks(g, 400):
            b.process_chunk(text, paired=paired, n_processed=base)
            base += text.count(b"\n+\n")
            b.bam_run()
            recs = []
            for k, r in enumerate(bam.split_records(b.bam_fetch()[0])):
                line = bam.decode_record(r[4:], names)
                lane = line.split(b":", 4)[3]
                tag = b"\tRG:Z:lane" + lane if k % 51 != 50 else b"\tRG:Z:other" if k % 102 == 50 else b""
                recs.append(bam.encode_record(line + (tag if line.split(b"\t")[0].count(b":") == 6 else b""), ref_id))
            runs.append(b"".join(recs))
    finally:
        b.close()
    marked, counts, rows = markdup.mark2(runs, HEADER_RG, DIST)
    return runs, marked, counts, rows


def test_simulated_batch(toy, simulated):                                        # noqa: F811
    _, ix = toy
    runs, marked, counts, rows = simulated
    assert sum(len(bam.split_records(r)) for r in runs) > 7000
    assert rows[0]["pair_optical_duplicates"] > 100 and rows[1]["pair_optical_duplicates"] > 30
    assert rows[0]["pair_duplicates"] > rows[0]["pair_optical_duplicates"] and rows[1]["unpaired_duplicates"] > 10
    assert rows[2]["pairs_examined"] + rows[2]["unpaired_examined"] > 0            # RG:Z:other and no RG: Unknown Library
    b = capi.Batch(ix, 100, 100 * 160)
    try:
        _, optical, got, want, _ = check_batch(b, b"".join(runs), HEADER_RG, DIST)
        assert got == want == markdup.mark2([b"".join(runs)], HEADER_RG, DIST)[2]
        assert sum(optical) == sum(r["pair_optical_duplicates"] for r in rows)
    finally:
        b.close()


def _sorter(tmp_path, tag, ix, runs, hdr, mem_bytes, setup, close):
    path = str(tmp_path / ("%s.bam" % tag))
    s = capi.Sorter(path, 0, hdr, tmp_prefix=str(tmp_path / ("%s_tmp" % tag)), mem_bytes=mem_bytes, markdup=True)
    b = capi.Batch(ix, 100, 100 * 160)
    try:
        setup(s)
        for k in np.random.default_rng(3).permutation(len(runs)):
            b.bam_upload(runs[k])
            s.put_batch(int(k), b)
            if k == 1:
                with pytest.raises(capi.BwamsError) as e:
                    s.set_markdup(None, 5)                                         # after a put
                assert e.value.code == ERR_ARG
    finally:
        st = close(s)
        b.close()
    return open(path, "rb").read(), open(path + ".bai", "rb").read(), st


def test_sorter_markdup_metrics(tmp_path, toy, simulated):                       # noqa: F811
    _, ix = toy
    runs, marked, counts, rows = simulated
    hdr = ix.bam_header(ix.sam_header(HEADER_RG.encode().rstrip(b"\n"), b"@PG\tID:bwa-mem2\tPN:bwa-mem2\n"))
    g = capi.DupGroups(HEADER_RG)
    mem = len(runs[0]) + len(runs[2])                                              # not all three fit: a spill
    d1, x1, st1 = _sorter(tmp_path, "libs", ix, runs, hdr, mem, lambda s: s.set_markdup(g, DIST), lambda s: s.close3())
    assert 0 < st1.spilled_runs < 3
    recs = gzip.decompress(d1)[len(hdr):]
    assert recs == bam.coord_sort(b"".join(marked))
    assert st1.dup.counts() == {k: counts[k] for k in st1.dup.counts()}
    assert rows_of(st1.lib) == rows
    text = capi.dup_metrics_text(g, st1.lib, "two lanes, one sorter")
    assert text == markdup.metrics_text(markdup.groups(HEADER_RG), rows, "two lanes, one sorter")
    assert text.count("\n") == 4 + 3 + 1 and "\nlibA\t" in text and "\nlibB\t" in text and "\nUnknown Library\t" in text
    assert bai.build(d1) == x1
    # without set_markdup: one library, today's file, through close2 and through close3
    legacy, lcounts = markdup.mark(runs)
    d2, x2, st2 = _sorter(tmp_path, "plain2", ix, runs, hdr, mem, lambda s: None, lambda s: s.close())
    d3, x3, st3 = _sorter(tmp_path, "plain3", ix, runs, hdr, mem, lambda s: None, lambda s: s.close3())
    assert gzip.decompress(d2)[len(hdr):] == bam.coord_sort(b"".join(legacy)) and d3 == d2 and x3 == x2 == bai.build(d2)
    assert st2.dup.counts() == st3.dup.counts() == {k: lcounts[k] for k in st2.dup.counts()}
    row = rows_of(st3.lib)
    assert len(row) == 1 and {k: row[0][k] for k in COUNTS4} == {k: lcounts[k] for k in COUNTS4}
    assert row[0]["pair_optical_duplicates"] == 0 and row[0]["unmapped"] == 0       # no table, no record-level counts kept
    assert d2 != d1
    s = capi.Sorter(str(tmp_path / "nomd.bam"), 0, hdr, markdup=False)
    with pytest.raises(capi.BwamsError) as e:
        s.set_markdup(g, DIST)                                                     # not opened with BWAMS_SORT_MARKDUP
    assert e.value.code == ERR_ARG
    s.close()
    g.close()
