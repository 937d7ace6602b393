"""The pileup's indel store on the GPU (csrc/pileup_indel.hip, csrc/api_pileup.hip, host/pileup_indel_vcf.cpp) through the C-ABI,
compared exactly with bwams/pileup.py's restatement of rules 14 to 17 and with the hand-written expectations of
tests/test_pileup_indels.py.  Every add runs twice, through the tiled path and under BWAMS_PILEUP_TILED=0: the indel kernels are the
same in both, and the counters and sums beside them must not notice."""
import ctypes as C
import gzip

import numpy as np
import pytest

from bwams import bam, capi, pileup, simulate
import test_pileup as T
import test_pileup_calls as TC
import test_pileup_indels as TI
from test_pileup import prec
from test_pileup_indels import R

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY = -3, -4
THRESHOLDS = ((-1, -1), (0, 1), (60, 4))              # (min_qual, min_depth) of the call comparisons; -1: the store's


@pytest.fixture
def way(monkeypatch):
    """way(tiled): the route of the adds that follow (BWAMS_PILEUP_TILED through bwams_debug_reload); the default again afterwards"""
    def set_(tiled: bool):
        monkeypatch.setenv("BWAMS_PILEUP_TILED", "1" if tiled else "0")
        capi.debug_reload()
    yield set_
    monkeypatch.undo()
    capi.debug_reload()


def same(got: capi.Pileup, want: pileup.Pileup, names, thresholds=THRESHOLDS):
    """every fetch, record and text against the restatement"""
    for k in range(len(want.regions)):
        assert np.array_equal(got.fetch(k), want.fetch(k)), k
        assert np.array_equal(got.fetch_span(k), want.fetch_span(k)), k
        if want.q is not None:
            assert np.array_equal(got.fetch_quality(k), want.fetch_quality(k)), k
    assert got.indel_alleles().tobytes() == want.indel_alleles().astype(capi.PILEUP_INDEL_ALLELE_DTYPE).tobytes()
    assert got.indel_info()["n_events"] == len(want.events)
    for q, d in thresholds:
        qd = (None if q < 0 else q, None if d < 0 else d)
        assert got.indel_calls(q, d).tobytes() == want.indel_calls(*qd).astype(capi.PILEUP_INDEL_DTYPE).tobytes(), (q, d)
        assert got.indel_vcf(names, "s", q, d) == want.indel_vcf(names, "s", *qd), (q, d)
        if want.q is not None:
            assert got.vcf_all(names, "s", -1, -1, q, d) == want.vcf_all(names, "s", None, None, *qd), (q, d)
            assert got.vcf(names, "s") == want.vcf(names, "s")


def both(way, l_ref, regions, adds, ref, opt=None, quality=True, **kw):
    """the restatement, and a device handle per route, after the same adds -> (want, tiled handle, direct handle)"""
    opt = opt or {}
    want = pileup.Pileup(l_ref, regions, **kw)
    if quality:
        want.set_quality()
    want.set_indels(**opt)
    n = [want.add(d) for d in adds]
    want.set_ref_genome(ref)
    out = []
    for tiled in (True, False):
        way(tiled)
        got = capi.Pileup(l_ref, regions, **kw)
        if quality:
            got.set_quality()
        got.set_indels(**opt)
        assert [got.add_records(d) for d in adds] == n
        for k, (r, b, e) in enumerate(want.regions):
            got.set_ref(k, np.minimum(ref[r][b:e], 4))
        out.append(got)
    return want, out[0], out[1]


def test_worked_example_and_hand_cases(way):
    want, a, b = both(way, T.EX_L_REF, (), [b"".join(T.EX_RECS)], [np.array(T.EX_REF, np.uint8)])
    for got in (a, b):
        assert got.fetch_span(0).tolist() == TI.EX_SPAN and [tuple(int(v) for v in x) for x in got.indel_alleles()] == TI.EX_ALLELES
        assert got.indel_vcf(T.EX_NAMES, "s1") == TI.EX_INDEL_VCF and got.vcf_all(T.EX_NAMES, "s1") == TI.EX_VCF_ALL
        assert got.vcf(T.EX_NAMES, "s1") == TC.EX_VCF and got.text(T.EX_NAMES) == T.EX_TEXT
        same(got, want, T.EX_NAMES)
        got.close()
    want, a, b = both(way, TI.HAND_L_REF, (), [b"".join(TI.HAND_RECS)], [np.array(TI.HAND_REF, np.uint8)], quality=False)
    for got in (a, b):
        assert [tuple(int(v) for v in x) for x in got.indel_alleles()] == TI.HAND_ALLELES and TI.as_tuples(got.indel_calls()) == TI.HAND_CALLS
        assert got.indel_vcf(TI.HAND_NAMES, "smp") == TI.HAND_VCF
        same(got, want, TI.HAND_NAMES)
        got.close()


@pytest.mark.parametrize("opt", TI.EDGE_CONFIGS)
def test_edges(way, opt):
    """tests/test_pileup_indels.py's edge records (test_edges there says what each is) under the default options, under max_len 1 with
    indel_q 50 and min_mapq 2, and under indel_q 0"""
    recs, ref = TI.edge_case()
    kw = {"min_mapq": 2} if "max_len" in opt else {}
    want, a, b = both(way, TI.EDGE_L_REF, TI.EDGE_REGIONS, [b"".join(recs)], ref, opt=opt, **kw)
    assert len(want.indel_alleles()) > 15 and len(want.indel_calls(0, 1)) > 8
    for got in (a, b):
        same(got, want, TI.EDGE_NAMES)
        got.close()


def test_many_alleles_and_contention(way):
    rng = np.random.default_rng(31)
    l_ref = [1200]
    recs = []
    for k in range(200):                                                        # 200 distinct alleles behind position 500: k in base 4 as four inserted bases
        recs.append(R(rng, 0, 496, "5M4I5M", ins=[1 << ((k >> (2 * j)) & 3) for j in range(4)], mapq=int(rng.integers(0, 61))))
    recs += [R(rng, 0, 596, "5M2D5M")] * 3 + [R(rng, 0, 596, "5M2I5M", ins=[2, 4])] * 3          # a tie in n between DEL and INS at 600
    recs += [R(rng, 0, 696, "5M2I5M", ins=[8, 1])] * 2 + [R(rng, 0, 696, "5M2I5M", ins=[2, 4])] * 2    # ... between two sequences at 700
    recs += [R(rng, 0, 296, "5M1D5M", mapq=k % 64) for k in range(5000)]         # 5000 records with one event on slot 300
    recs += [R(rng, 0, 1019, "5M1I5M", ins=[1]), R(rng, 0, 1020, "5M1D5M"), R(rng, 0, 1019, "5M1D5M"), R(rng, 0, 1020, "5M1I5M", ins=[4])]      # slots 1023 and 1024
    ref = [rng.integers(0, 4, 1200).astype(np.uint8)]
    want, a, b = both(way, l_ref, (), [b"".join(recs)], ref)
    al = want.indel_alleles()
    assert (al["pos"] == 500).sum() == 200 and int(al[al["pos"] == 300]["n"][0]) == 5000
    calls = {int(c["pos"]): c for c in want.indel_calls(0, 1)}
    assert int(calls[600]["type"]) == pileup.EV_DEL and int(calls[600]["n_other"]) == 3
    assert (int(calls[700]["seq"]), int(calls[700]["n_alt"]), int(calls[700]["n_other"])) == (0b0011, 2, 2)      # TA is the word 3, CG the word 9
    assert {1023, 1024} <= set(calls)
    for got in (a, b):
        same(got, want, [b"m"])
        got.close()


def _long_cigar(rng, pos, n_ops=300):
    ops = []
    for k in range(n_ops // 2):
        ops += [(3, 0), (1, 1 if k % 3 else 2)]
    ops += [(3, 0)] * (n_ops - len(ops))
    codes = [int(c) for c in rng.choice([1, 2, 4, 8], sum(n for n, op in ops if op in (0, 1)))]
    return prec(0, pos, ops, codes)


def test_long_cigars(way):
    """a record of 300 ops, 3M alternating with 1I or 1D, alone and among short records: the walk is over ops, whatever their number"""
    rng = np.random.default_rng(37)
    l_ref = [2000]
    ref = [rng.integers(0, 5, 2000).astype(np.uint8)]
    long_ = _long_cigar(rng, 100)
    short = [R(rng, 0, int(rng.integers(0, 1900)), "20M1I20M") for _ in range(100)]
    for recs in ([long_], short[:50] + [long_, _long_cigar(rng, 700, 65), _long_cigar(rng, 900, 64)] + short[50:]):
        want, a, b = both(way, l_ref, (), [b"".join(recs)], ref)
        assert len(want.events) >= 150
        for got in (a, b):
            same(got, want, [b"l"])
            got.close()


@pytest.mark.parametrize("seed", (1, 2))
def test_random(way, seed):
    """tests/test_pileup_indels.py::test_random_inputs_say_something holds the conditions on these inputs"""
    recs, ref = TI.random_case(seed)
    want, a, b = both(way, TI.RAND_L_REF, TI.RAND_REGIONS, [b"".join(recs)], ref)
    assert len(want.indel_calls()) >= 20
    for got in (a, b):
        same(got, want, TI.RAND_NAMES)
        got.close()


def test_accumulation_growth_and_reset(way):
    recs, ref = TI.random_case(3, 1500)
    whole = b"".join(recs)
    fifth = [b"".join(recs[k * len(recs) // 5:(k + 1) * len(recs) // 5]) for k in range(5)]
    want, a, b = both(way, TI.RAND_L_REF, TI.RAND_REGIONS, [whole], ref)
    alleles = want.indel_alleles().astype(capi.PILEUP_INDEL_ALLELE_DTYPE).tobytes()
    for got in (a, b):
        same(got, want, TI.RAND_NAMES, THRESHOLDS[:1])
        got.close()
    L = capi.lib()
    for adds in (fifth, [b"".join(recs[::-1])]):
        _, a, b = both(way, TI.RAND_L_REF, TI.RAND_REGIONS, adds, ref)
        for got in (a, b):
            same(got, want, TI.RAND_NAMES, THRESHOLDS[:1])
            got.close()
    # growth: a first add of few events sizes the buffer at its least; the later ones outgrow it, and what it held is kept
    way(True)
    got = capi.Pileup(TI.RAND_L_REF, TI.RAND_REGIONS)
    got.set_quality()
    got.set_indels()
    got.add_records(b"".join(recs[:40]))
    first = got.indel_info()
    held = got.indel_alleles().tobytes()
    assert 0 < first["n_events"] == first["n_appended"] <= first["cap_events"] == 256 and len(held) > 0
    got.add_records(b"".join(recs[40:]))
    info = got.indel_info()
    assert info["cap_events"] > 256 and info["n_events"] == len(want.events) > 256 and info["n_appended"] == info["n_events"] - first["n_events"]
    for k, (r, x, e) in enumerate(want.regions):
        got.set_ref(k, np.minimum(ref[r][x:e], 4))
    assert got.indel_alleles().tobytes() == alleles
    same(got, want, TI.RAND_NAMES, THRESHOLDS[:1])
    # _set_indels after an add is refused and touches nothing; an add that rule 3 refuses leaves everything as it was
    assert L.bwams_pileup_set_indels(got.h, None) == ERR_ARG and "not zero" in L.bwams_last_error().decode()
    counted = got.info()["n_counted"]
    with pytest.raises(capi.BwamsError) as e:
        got.add_records(recs[0] + prec(0, 200, "3M1I3M", "ACGTAC"))             # the CIGAR asks for 7 bases
    assert e.value.code == ERR_ARG and got.indel_info()["n_events"] == info["n_events"] and got.info()["n_counted"] == counted
    same(got, want, TI.RAND_NAMES, THRESHOLDS[:1])
    got.reset()
    assert got.indel_info()["n_events"] == 0 and len(got.indel_alleles()) == 0 and len(got.indel_calls(0, 1)) == 0
    assert not any(got.fetch_span(k).any() or got.fetch(k).any() for k in range(len(want.regions)))
    got.set_indels(min_qual=0, indel_q=13, max_len=2)                           # directly after a reset: other options
    got.add_records(fifth[1])
    after = pileup.Pileup(TI.RAND_L_REF, TI.RAND_REGIONS)
    after.set_quality()
    after.set_indels(min_qual=0, indel_q=13, max_len=2)
    after.add(fifth[1])
    after.set_ref_genome(ref)
    same(got, after, TI.RAND_NAMES)
    got.close()


def test_arguments_and_capacity(way):
    L = capi.lib()
    way(True)
    p = capi.Pileup(TI.HAND_L_REF)
    n = C.c_int64(-1)
    buf = np.zeros(64, capi.PILEUP_INDEL_DTYPE)
    vp = buf.ctypes.data_as(C.c_void_p)
    out = C.create_string_buffer(8192)
    info = capi.PileupIndelInfo()
    assert L.bwams_pileup_fetch_span(p.h, 0, 0, 4, vp) == ERR_ARG               # no store yet
    assert "no indel store" in L.bwams_last_error().decode() or "indel store" in L.bwams_last_error().decode()
    assert L.bwams_pileup_indel_alleles(p.h, None, 0, C.byref(n)) == ERR_ARG
    assert L.bwams_pileup_indel_calls(p.h, -1, -1, None, 0, C.byref(n)) == ERR_ARG
    assert L.bwams_pileup_indel_vcf(p.h, b"h\0", b"s", -1, -1, out, 8192, C.byref(n)) == ERR_ARG
    assert L.bwams_pileup_vcf_all(p.h, b"h\0", b"s", -1, -1, -1, -1, out, 8192, C.byref(n)) == ERR_ARG
    assert L.bwams_pileup_indel_info(p.h, C.byref(info)) == ERR_ARG
    for o in (capi.PileupIndelOpt(-1, 1, 40, 32, 0), capi.PileupIndelOpt(20, 0, 40, 32, 0), capi.PileupIndelOpt(20, 1, -1, 32, 0),
              capi.PileupIndelOpt(20, 1, 94, 32, 0), capi.PileupIndelOpt(20, 1, 40, 0, 0), capi.PileupIndelOpt(20, 1, 40, 33, 0),
              capi.PileupIndelOpt(20, 1, 40, 32, 1)):
        assert L.bwams_pileup_set_indels(p.h, C.byref(o)) == ERR_ARG
    assert L.bwams_pileup_set_indels(None, None) == ERR_ARG
    assert L.bwams_pileup_fetch_span(p.h, 0, 0, 4, vp) == ERR_ARG               # a refused call made no store
    assert L.bwams_pileup_set_indels(p.h, None) == 0                            # NULL: {20, 1, 40, 32, 0}
    assert L.bwams_pileup_vcf_all(p.h, b"h\0", b"s", -1, -1, -1, -1, out, 8192, C.byref(n)) == ERR_ARG      # the store alone: no quality plane
    assert "no quality plane" in L.bwams_last_error().decode()
    assert L.bwams_pileup_indel_alleles(p.h, None, 0, C.byref(n)) == 0 and n.value == 0          # an empty store answers
    assert p.indel_vcf(TI.HAND_NAMES, "smp") == TI.VCF_HEAD % ("##contig=<ID=h,length=16>\n", "smp")
    p.set_indels()                                                              # twice while the counters are zero
    p.add_records(b"".join(TI.HAND_RECS))
    p.set_ref(0, TI.HAND_REF)
    assert L.bwams_pileup_indel_info(p.h, C.byref(info)) == 0 and (info.n_events, info.n_appended) == (5, 5)
    assert L.bwams_pileup_indel_info(p.h, None) == ERR_ARG and L.bwams_pileup_indel_info(None, C.byref(info)) == ERR_ARG
    assert L.bwams_pileup_indel_calls(p.h, -1, -1, None, 0, C.byref(n)) == 0 and n.value == 2    # NULL: the count
    assert L.bwams_pileup_indel_calls(p.h, -1, -1, None, 0, None) == 0                           # ... which nobody has to want
    assert L.bwams_pileup_indel_calls(p.h, -1, -1, vp, 1, C.byref(n)) == ERR_CAPACITY and n.value == 2
    with pytest.raises(capi.BwamsError) as e:
        p.indel_calls(cap=1)
    assert e.value.code == ERR_CAPACITY and p.n_indel_calls == 2 and TI.as_tuples(p.indel_calls(cap=2)) == TI.HAND_CALLS
    assert L.bwams_pileup_indel_calls(p.h, -1, 0, vp, 64, C.byref(n)) == ERR_ARG                 # min_depth 0
    assert L.bwams_pileup_indel_calls(p.h, 1000, -1, vp, 0, C.byref(n)) == 0 and n.value == 0
    assert L.bwams_pileup_indel_calls(p.h, -1, -1, vp, -1, C.byref(n)) == ERR_ARG
    abuf = np.zeros(8, capi.PILEUP_INDEL_ALLELE_DTYPE)
    ap = abuf.ctypes.data_as(C.c_void_p)
    assert L.bwams_pileup_indel_alleles(p.h, None, 0, C.byref(n)) == 0 and n.value == 3
    assert L.bwams_pileup_indel_alleles(p.h, ap, 2, C.byref(n)) == ERR_CAPACITY and n.value == 3
    assert L.bwams_pileup_indel_alleles(p.h, ap, -1, C.byref(n)) == ERR_ARG
    assert L.bwams_pileup_indel_alleles(p.h, ap, 8, None) == 0 and [tuple(int(v) for v in x) for x in abuf[:3]] == TI.HAND_ALLELES
    with pytest.raises(capi.BwamsError) as e:
        p.indel_alleles(cap=2)
    assert e.value.code == ERR_CAPACITY and p.n_alleles == 3
    assert L.bwams_pileup_indel_vcf(p.h, b"h\0", b"smp", -1, -1, None, 0, C.byref(n)) == ERR_CAPACITY and n.value == len(TI.HAND_VCF)
    assert L.bwams_pileup_indel_vcf(p.h, b"h\0", b"smp", -1, -1, out, len(TI.HAND_VCF) - 1, C.byref(n)) == ERR_CAPACITY
    assert L.bwams_pileup_indel_vcf(p.h, b"h\0", b"smp", -1, -1, out, 8192, C.byref(n)) == 0 and out.raw[:n.value].decode() == TI.HAND_VCF
    assert L.bwams_pileup_indel_vcf(p.h, None, b"smp", -1, -1, out, 8192, C.byref(n)) == ERR_ARG
    assert L.bwams_pileup_indel_vcf(p.h, b"h\0", None, -1, -1, out, 8192, C.byref(n)) == ERR_ARG
    assert L.bwams_pileup_indel_vcf(p.h, b"h\0", b"smp", -1, 0, out, 8192, C.byref(n)) == ERR_ARG
    for region, beg, end in ((1, 0, 1), (-1, 0, 1), (0, 0, 17), (0, 5, 4), (0, -1, 2)):
        assert L.bwams_pileup_fetch_span(p.h, region, beg, end, vp) == ERR_ARG, (region, beg, end)
    assert L.bwams_pileup_fetch_span(p.h, 0, 0, 4, None) == ERR_ARG
    assert p.fetch_span(0, 3, 3).shape == (0, 4) and p.fetch_span(0, 4, 5).tolist() == [[3, 120, 0, 903]]
    p.close()
    q = capi.Pileup(TI.HAND_L_REF)                                              # the plane alone: no store
    q.set_quality()
    assert L.bwams_pileup_vcf_all(q.h, b"h\0", b"s", -1, -1, -1, -1, out, 8192, C.byref(n)) == ERR_ARG
    q.set_indels()
    assert L.bwams_pileup_vcf_all(q.h, b"h\0", b"s", -1, -1, -1, -1, None, 0, C.byref(n)) == ERR_CAPACITY
    assert n.value == len(TI.VCF_HEAD % ("##contig=<ID=h,length=16>\n", "s"))
    assert L.bwams_pileup_vcf_all(q.h, None, b"s", -1, -1, -1, -1, out, 8192, C.byref(n)) == ERR_ARG
    assert L.bwams_pileup_vcf_all(q.h, b"h\0", b"s", -1, 0, -1, -1, out, 8192, C.byref(n)) == ERR_ARG
    assert L.bwams_pileup_vcf_all(q.h, b"h\0", b"s", -1, -1, -1, 0, out, 8192, C.byref(n)) == ERR_ARG
    q.close()


def test_unchanged_without_and_with_the_store(way):
    recs, ref = TI.random_case(4, 1200)
    data = b"".join(recs)
    for tiled in (True, False):
        way(tiled)
        plain, with_i = capi.Pileup(TI.RAND_L_REF, TI.RAND_REGIONS), capi.Pileup(TI.RAND_L_REF, TI.RAND_REGIONS)
        plain.set_quality()
        with_i.set_quality()
        with_i.set_indels()
        assert plain.add_records(data) == with_i.add_records(data)
        for h in (plain, with_i):
            for k, (r, b, e) in enumerate(h.regions):
                h.set_ref(k, np.minimum(ref[r][b:e], 4))
        for k in range(len(plain.regions)):
            assert plain.fetch(k).tobytes() == with_i.fetch(k).tobytes() and plain.fetch_quality(k).tobytes() == with_i.fetch_quality(k).tobytes()
        assert plain.fetch(0).any() and with_i.indel_info()["n_events"] > 100
        for pair in ((2, 200), (1, 0)):
            assert plain.sites(*pair).tobytes() == with_i.sites(*pair).tobytes() and len(plain.sites(*pair)) > 5
            assert plain.text(TI.RAND_NAMES, *pair) == with_i.text(TI.RAND_NAMES, *pair)
        assert plain.calls(0, 1).tobytes() == with_i.calls(0, 1).tobytes() and len(plain.calls(0, 1)) > 5
        assert plain.vcf(TI.RAND_NAMES, "s", 0, 1) == with_i.vcf(TI.RAND_NAMES, "s", 0, 1)
        i, j = plain.info(), with_i.info()
        assert all(i[k] == j[k] for k in ("tile", "n_slots", "n_counted", "n_entries", "n_direct"))
        plain.close(); with_i.close()


def test_sorter(tmp_path):
    """a handle with the quality plane and the indel store set on a sorted writer: after the close _vcf_all is the restatement's over
    the records as written, and the file and its index are byte for byte those of a sorter without the handle"""
    from test_gpu_pileup import _sorter
    rng = np.random.default_rng(29)
    g = simulate.make_genome(20000, seed=2, repeat_frac=0.0)
    ix = capi.Index.build(g, 0)
    l_ref = [1500]
    hdr = bam.header_block(b"@HD\tVN:1.6\tSO:coordinate\n", [b"s0"], l_ref)
    ref = rng.integers(0, 4, 1500).astype(np.uint8)
    recs = []
    for k in range(80):
        pos = int(rng.integers(0, 1400))
        a = 20 + 10 * (pos % 4)                                                # the indel of a read depends on where it starts: alleles repeat
        cigar = ["80M", "%dM2D%dM" % (a, 80 - a), "%dM1I%dM" % (a, 79 - a)][k % 3]
        recs.append(R(rng, 0, pos, cigar, ins=[4] if k % 3 == 2 else None, qual=[int(q) for q in rng.integers(5, 41, 80)], flag=16 * (k % 2),
                      mapq=int(rng.choice([20, 40, 60])), name=b"f%d" % k))
    runs = [b"".join(recs[0::2]), b"".join(recs[1::2])]
    try:
        p = capi.Pileup(l_ref)
        p.set_quality(min_qual=0)
        p.set_indels(min_qual=0)
        data0, x0, _ = _sorter(tmp_path, "plain", ix, hdr, runs)
        data1, x1, st = _sorter(tmp_path, "indels", ix, hdr, runs, p=p)
        assert data0 == data1 and x0 == x1
        p.set_ref(0, ref)
        written = gzip.decompress(data0)[len(hdr):]
        want = pileup.Pileup(l_ref)
        want.set_quality(min_qual=0)
        want.set_indels(min_qual=0)
        want.add(written)
        want.set_ref(0, ref)
        assert len(want.indel_calls()) > 10 and len(want.calls()) > 10
        same(p, want, [b"s0"])
        p.close()
    finally:
        ix.close()
