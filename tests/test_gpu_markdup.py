"""Duplicate marking on the GPU (csrc/markdup.hip: bwams_bam_templates / _templates_fetch, bwams_dup_decide, bwams_bam_markdup) and in
the sorted BAM writer (host/bam_sort.cpp: BWAMS_SORT_MARKDUP) against bwams/markdup.py's restatement of the rules and the hand-written
expectations of tests/test_markdup.py."""
import ctypes as C
import gzip
import struct
import threading

import numpy as np
import pytest

from bwams import bai, bam, bgzf, capi, markdup, simulate
from test_markdup import CASES, REFUSALS, D, flags, qlen

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -3, -6


@pytest.fixture(scope="module")
def toy():
    g = simulate.make_genome(400000, seed=61, repeat_frac=0.0)
    ix = capi.Index.build(g, 0)
    contigs = np.zeros(2, capi.CONTIG_DTYPE)
    contigs["offset"], contigs["len"] = [0, 150000], [150000, len(g) - 150000]
    ix.set_contigs(contigs)
    ix.set_contig_names(["chrA", "chrB"])
    yield g, ix
    ix.close()


def _counts(st) -> dict:
    return {k: v for k, v in st.counts().items()}


def test_hand_built_cases(toy):
    _, ix = toy
    b = capi.Batch(ix, 100, 100 * 160)
    try:
        for name, recs, want, counts in CASES:
            data = b"".join(recs)
            assert b.bam_upload(data) == len(recs)
            st = b.bam_markdup()
            out, _ = b.bam_fetch()
            assert [f & D for f in flags(out)] == want, name
            assert [f & ~D for f in flags(out)] == [f & ~D for f in flags(data)], name
            assert _counts(st) == counts, name
            assert b.bam_markdup().records_marked == counts["records_marked"] and b.bam_fetch()[0] == out     # twice: the same
            n_t, n_e = b.bam_templates()
            ends, rt = b.bam_templates_fetch()
            wn, wends, wrt = markdup.ends(recs)
            assert n_t == wn and rt.tolist() == wrt and n_e == len(wends), name
            assert [dict((k, int(e[k])) for k in wends[0]) for e in ends] == wends, name
            dup, dst = capi.dup_decide(0, ends, n_t)
            wdup, wcounts = markdup.decide(wends, n_t)
            assert dup.tolist() == [int(x) for x in wdup] and _counts(dst) == wcounts, name
        L = capi.lib()
        nt, ne = C.c_int64(0), C.c_int64(0)
        for name, recs, at, why in REFUSALS:
            b.bam_upload(b"".join(recs))
            assert L.bwams_bam_templates(b.h, C.byref(nt), C.byref(ne)) == ERR_UNSUPPORTED, name
            assert L.bwams_last_error().decode().startswith("bwams_bam_templates: record %d: %s" % (at, markdup.REASONS[why])), name
            assert L.bwams_bam_markdup(b.h, None) == ERR_UNSUPPORTED, name
        bad = np.zeros(1, capi.DUP_END_DTYPE)
        bad["tmpl"] = 5
        with pytest.raises(capi.BwamsError) as e:
            capi.dup_decide(0, bad, 5)                                        # tmpl outside [0, n_templates)
        assert e.value.code == ERR_ARG
    finally:
        b.close()


def _fq(reads, names, quals) -> bytes:
    return b"".join(b"@%s\n%s\n+\n%s\n" % (n, bytes(b"ACGTN"[c] for c in r), q * len(r)) for r, n, q in zip(reads, names, quals))


def _se_chunk(g, n, seed):
    """single-end reads with planted duplicates: renamed copies with lower qualities, and 3'-trimmed copies; -> (text, copy names)"""
    rng = np.random.default_rng(seed)
    reads, _, _ = simulate.make_reads(g, n, seed=seed)
    rs, nm, qs, planted = [], [], [], []
    for i, r in enumerate(reads):
        rs.append(r); nm.append(b"s%d" % i); qs.append(b"I")
        if i % 7 == 0:
            rs.append(r); nm.append(b"s%d_copy" % i); qs.append(b"5"); planted.append(nm[-1])
        if i % 11 == 0:
            rs.append(r[:int(rng.integers(100, 140))]); nm.append(b"s%d_trim" % i); qs.append(b"I"); planted.append(nm[-1])
    return _fq(rs, nm, qs), planted


def _pe_chunk(g, n, seed, prefix=b"p"):
    """pairs with planted duplicates: renamed copies with lower qualities, and copies whose second end is random sequence"""
    rng = np.random.default_rng(seed)
    pr = simulate.make_read_pairs(g, n, seed=seed, damaged_frac=0.0, discordant_frac=0.0)
    e1, e2, nm, qs, planted = [], [], [], [], []
    for i in range(n):
        a, c = pr[2 * i], pr[2 * i + 1]
        e1.append(a); e2.append(c); nm.append(prefix + b"%d" % i); qs.append(b"I")
        if i % 5 == 0:
            e1.append(a); e2.append(c); nm.append(prefix + b"%d_copy" % i); qs.append(b"5"); planted.append(nm[-1])
        if i % 9 == 0:
            e1.append(a); e2.append(rng.integers(0, 4, len(c)).astype(np.uint8)); nm.append(prefix + b"%d_half" % i); qs.append(b"I")
            planted.append(nm[-1])
    return _fq(e1, nm, qs), _fq(e2, nm, qs), planted


def _check_batch(b, planted):
    """the batch's marked records == markdup.mark of its unmarked records; every planted copy's mapped primary marked; sorting before
    and after the marking gives the same bytes"""
    b.bam_run()
    rec0, _ = b.bam_fetch()
    b.bam_sort()
    (want,), counts = markdup.mark([rec0])
    st = b.bam_markdup()
    got, _ = b.bam_fetch()
    assert got == want
    assert _counts(st) == {k: counts[k] for k in _counts(st)}
    srt, _ = b.bam_sorted_fetch()                                              # sorted before the marking, marked in place
    b.bam_run()
    b.bam_markdup()
    b.bam_sort()                                                               # sorted after it
    assert b.bam_sorted_fetch()[0] == srt == bam.coord_sort(want)
    mapped = {}                                                                # name -> FLAG of its first mapped primary
    for r in bam.split_records(want):
        f = struct.unpack_from("<H", r, 18)[0]
        if not f & 0x904:
            mapped.setdefault(r[36:36 + r[12] - 1], f)
    checked = [n for n in planted if n in mapped and n.rsplit(b"_", 1)[0] in mapped]     # a copy of a read that maps, mapped itself
    assert len(checked) >= 0.95 * len(planted)
    assert all(mapped[n] & D for n in checked)
    assert counts["unpaired_duplicates"] + counts["pair_duplicates"] >= len(checked)
    return want, counts


def test_simulated_single_end(toy):
    g, ix = toy
    text, planted = _se_chunk(g, 3000, 5)
    b = capi.Batch(ix, 4000, 4000 * 160)
    try:
        b.process_chunk(text)
        _, counts = _check_batch(b, planted)
        assert counts["pairs_examined"] == 0 and counts["unpaired_duplicates"] > 0
    finally:
        b.close()


def test_simulated_paired_end(toy):
    g, ix = toy
    t1, t2, planted = _pe_chunk(g, 1500, 8)
    b = capi.Batch(ix, 4000, 4000 * 160)
    try:
        b.process_chunk2(t1, t2)
        _, counts = _check_batch(b, planted)
        assert counts["pair_duplicates"] > 0 and counts["unpaired_duplicates"] > 0
    finally:
        b.close()


def _sorter_run(tmp_path, tag, ix, texts, hdr, mem_bytes, md):
    """every chunk in a batch of its own, put_batch from two threads in shuffled seq order"""
    path = str(tmp_path / ("%s.bam" % tag))
    s = capi.Sorter(path, 0, hdr, tmp_prefix=str(tmp_path / ("%s_tmp" % tag)), mem_bytes=mem_bytes, markdup=md)
    bs, runs = [], []
    try:
        base = 0
        for t in texts:
            b = capi.Batch(ix, 1500, 1500 * 160)
            bs.append(b)
            b.process_chunk(t, paired=True, n_processed=base)
            base += t.count(b"\n+\n")
            b.bam_run()
            runs.append(b.bam_fetch()[0])
        order = list(np.random.default_rng(len(tag)).permutation(len(texts)))
        errs = []

        def put(items):
            try:
                for i in items:
                    s.put_batch(int(i), bs[i])
            except Exception as e:                                             # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=put, args=(order[k::2],)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        if md:
            with pytest.raises(capi.BwamsError) as e:                          # sorted host records carry no templates
                bs[0].bam_sort()                                               # sorted already: at once
                s.put(len(texts), *bs[0].bam_sorted_fetch())
            assert e.value.code == ERR_ARG
    finally:
        st = s.close()
        for b in bs:
            b.close()
    return open(path, "rb").read(), open(path + ".bai", "rb").read(), st, runs


def _by_member(x: bytes, data: bytes) -> dict:
    """the index with every virtual offset as (member ordinal, offset in the member's data), counts kept as they are"""
    at = {off: k for k, (off, *_) in enumerate(bgzf.walk(data))}
    v = lambda o: (at[o >> 16], o & 0xFFFF)                                     # noqa: E731
    idx = bai.read(x)
    for r in idx["refs"]:
        for b_, ch in r["bins"].items():
            r["bins"][b_] = [(v(a), v(e)) for a, e in ch] if b_ != bai.PSEUDO_BIN else [(v(ch[0][0]), v(ch[0][1])), ch[1]]
        r["lin"] = [v(o) for o in r["lin"]]
    return idx


def test_sorter_markdup(tmp_path, toy):
    g, ix = toy
    texts = []
    first = None
    for c in range(5):
        t1, t2, _ = _pe_chunk(g, 400, 30 + c, prefix=b"c%d_" % c)
        l1, l2 = t1.split(b"\n"), t2.split(b"\n")
        recs = [b"\n".join(l1[4 * i:4 * i + 4] + l2[4 * i:4 * i + 4]) + b"\n" for i in range(len(l1) // 4)]
        if c == 0:
            first = recs[0]
        if c == 3:                                                             # a duplicate of chunk 0's first pair, renamed, lower qualities
            x = first.split(b"\n")
            recs.insert(7, b"\n".join([b"@planted", x[1], b"+", b"5" * len(x[1]), b"@planted", x[5], b"+", b"5" * len(x[5])]) + b"\n")
        texts.append(b"".join(recs))
    hdr = ix.bam_header(ix.sam_header(None, b"@PG\tID:bwa-mem2\tPN:bwa-mem2\n"))
    d1, x1, st1, runs = _sorter_run(tmp_path, "mem", ix, texts, hdr, 1 << 40, True)
    d2, x2, st2, runs2 = _sorter_run(tmp_path, "spill", ix, texts, hdr, 0, True)
    d0, x0, st0, _ = _sorter_run(tmp_path, "plain", ix, texts, hdr, 1 << 40, False)
    assert runs == runs2 and st1.spilled_runs == 0 and st2.spilled_runs == len(texts)
    assert d1 == d2 and x1 == x2 and bai.build(d1) == x1
    assert _by_member(x1, d1) == _by_member(x0, d0)          # the same index but for the members' compressed sizes: 0x400 moves no record
    marked, counts = markdup.mark(runs)
    recs = gzip.decompress(d1)[len(hdr):]
    assert recs == bam.coord_sort(b"".join(marked))
    assert gzip.decompress(d0)[len(hdr):] == bam.coord_sort(b"".join(runs))   # without the flag FLAG passes through
    assert _counts(st1.dup) == {k: counts[k] for k in _counts(st1.dup)} and _counts(st2.dup) == _counts(st1.dup)
    assert st0.dup.templates == 0 and st1.dup.ms_decide > 0
    pl = [r for r in bam.split_records(recs) if r[36:36 + r[12] - 1] == b"planted"]
    assert len(pl) == 2 and all(struct.unpack_from("<H", r, 18)[0] & D for r in pl)


def test_200k_templates_upload(toy):
    _, ix = toy
    rng = np.random.default_rng(17)
    ref_id = {b"c%d" % i: i for i in range(3)}
    cig = [b"100M", b"5S95M", b"95M5S", b"3H97M", b"90M10H", b"50M2D50M", b"2S40M3I55M"]
    lines = []
    n = 200000
    for t in range(n):
        name = b"t%d" % t
        kind = rng.integers(0, 10)
        q = lambda: bytes(rng.integers(35, 75, 100).astype(np.uint8)) if rng.random() > 0.05 else b"*"   # noqa: E731

        def ln(flag, rid, pos, c):
            n_q = qlen(c)
            qq = q()
            return b"\t".join([name, b"%d" % flag, b"c%d" % rid, b"%d" % (pos + 1), b"60", c, b"*", b"0", b"0", b"A" * n_q,
                               qq[:n_q] if qq != b"*" else b"*"])
        pos = lambda: int(rng.integers(0, 3000))                                 # noqa: E731
        if kind < 4:                                                            # a fragment
            lines.append(ln(16 * int(rng.integers(0, 2)), int(rng.integers(0, 3)), pos(), cig[rng.integers(0, len(cig))]))
        elif kind < 9:                                                          # a pair, either end first, sometimes a supplementary
            rid, p1 = int(rng.integers(0, 3)), pos()                           # the mate a few inserts away: pairs collide too
            a = ln(0x1 | 0x40 | 16 * int(rng.integers(0, 2)), rid, p1, cig[rng.integers(0, len(cig))])
            c = ln(0x1 | 0x80 | 16 * int(rng.integers(0, 2)), rid, p1 + 100 * int(rng.integers(0, 4)), cig[rng.integers(0, len(cig))])
            lines += [a, c] if rng.random() < 0.5 else [c, a]
            if rng.random() < 0.1:
                lines.append(ln(0x1 | 0x40 | 0x800, 0, pos(), b"30H70M"))
        else:                                                                   # a pair with its last end unmapped
            lines.append(ln(0x1 | 0x40 | 0x8, int(rng.integers(0, 3)), pos(), b"100M"))
            lines.append(b"\t".join([name, b"%d" % (0x1 | 0x80 | 0x4), b"*", b"0", b"0", b"*", b"*", b"0", b"0", b"ACGT", b"IIII"]))
    data = b"".join(bam.encode_record(x, ref_id) for x in lines)
    b = capi.Batch(ix, 1000, 1000 * 160)
    try:
        assert b.bam_upload(data) == len(lines)
        st = b.bam_markdup()
        (want,), counts = markdup.mark([data])
        assert b.bam_fetch()[0] == want
        assert _counts(st) == {k: counts[k] for k in _counts(st)} and st.templates == n
        assert counts["pair_duplicates"] > 1000 and counts["unpaired_duplicates"] > 1000
    finally:
        b.close()
