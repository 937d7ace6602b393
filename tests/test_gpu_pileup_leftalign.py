"""Rule 18 on the GPU (pileup_indel_run_kernel and pileup_indel_align_kernel in csrc/pileup_indel.hip, csrc/api_pileup.hip) through the
C-ABI: every fetch, record and text compared exactly with bwams/pileup.py's restatement, which tests/test_pileup_leftalign.py pins
from first principles and whose inputs these are.  Every add runs through the tiled route and under BWAMS_PILEUP_TILED=0; on a
left-aligning handle the reference goes in before the records."""
import ctypes as C
import gzip

import numpy as np
import pytest

from bwams import bam, capi, pileup, simulate
import test_pileup as T
import test_pileup_indels as TI
import test_pileup_leftalign as TL
from test_gpu_pileup_indels import THRESHOLDS, same, way       # noqa: F401  (way is a fixture)

pytestmark = pytest.mark.gpu

ERR_ARG = -3


def handle(l_ref, regions, ref, adds, leftalign=True, quality=False, opt=None, **kw) -> capi.Pileup:
    """a device handle after the adds, made as TL.model makes the restatement: the option, the reference, then the records"""
    got = capi.Pileup(l_ref, regions, **kw)
    if quality:
        got.set_quality()
    got.set_indels(**(opt or {}))
    if leftalign is not None:
        got.set_indel_leftalign(leftalign)
    for k, (r, b, e) in enumerate(got.regions):
        got.set_ref(k, np.minimum(ref[r][b:e], 4))
    for d in adds:
        got.add_records(d)
    return got


def check(way, names, l_ref, regions, ref, adds, thresholds=THRESHOLDS, **kw) -> pileup.Pileup:
    """both routes against the restatement; no span sum wrapped below zero"""
    want = TL.model(l_ref, regions, ref, adds, **kw)
    for tiled in (True, False):
        way(tiled)
        got = handle(l_ref, regions, ref, adds, **kw)
        same(got, want, names, thresholds)
        for k in range(len(want.regions)):
            assert not (got.fetch_span(k) >= 2 ** 31).any(), k
        got.close()
    return want


def test_hand_cases(way):
    p = check(way, TL.A10_NAMES, TL.A10_L_REF, (), [TL.A10_REF], [b"".join(TL.A10_RECS)])
    assert TL.alleles(p) == TL.A10_ALLELES and p.indel_vcf(TL.A10_NAMES, "s") == TL.A10_VCF
    p = check(way, TL.CA8_NAMES, TL.CA8_L_REF, (), [TL.CA8_REF], [b"".join(TL.CA8_RECS)])
    assert TL.alleles(p) == TL.CA8_ALLELES and p.indel_vcf(TL.CA8_NAMES, "s") == TL.CA8_VCF
    p = check(way, TL.C2_NAMES, TL.C2_L_REF, (), [TL.C2_REF], [b"".join(TL.C2_RECS)])
    assert p.indel_vcf(TL.C2_NAMES, "s1") == TL.C2_HEAD + TL.C2_ROW
    p = check(way, T.EX_NAMES, T.EX_L_REF, (), [np.array(T.EX_REF, np.uint8)], [b"".join(T.EX_RECS)], quality=True)
    assert p.indel_vcf(T.EX_NAMES, "s1") == TI.EX_INDEL_VCF and p.vcf_all(T.EX_NAMES, "s1") == TI.EX_VCF_ALL
    for tiled in (True, False):                                                 # the literals against the device itself
        way(tiled)
        got = handle(TL.A10_L_REF, (), [TL.A10_REF], [b"".join(TL.A10_RECS)])
        assert got.fetch_span(0).tolist() == [[n, 40 * n, 0, 301 * n] for n in TL.A10_SPAN_N]
        assert [tuple(int(v) for v in a) for a in got.indel_alleles()] == TL.A10_ALLELES and got.indel_vcf(TL.A10_NAMES, "s") == TL.A10_VCF
        got.close()
        got = handle(TL.CA8_L_REF, (), [TL.CA8_REF], [b"".join(TL.CA8_RECS)])
        assert got.fetch_span(0)[:, 0].tolist() == TL.CA8_SPAN_N and got.indel_vcf(TL.CA8_NAMES, "s") == TL.CA8_VCF
        assert [tuple(int(v) for v in a) for a in got.indel_alleles()] == TL.CA8_ALLELES
        got.close()


def test_shifts_across_the_64_position_step(way):
    """shifts of 63, 64, 65, 128, 129 and one more each; a 200-base homopolymer; a 300-base (CA)n with deletions and insertions
    (tests/test_pileup_leftalign.py::test_step_case_crosses_the_steps holds the shifts)"""
    l_ref, regions, ref, recs, _ = TL.step_case()
    check(way, [b"x"], l_ref, regions, ref, [b"".join(recs)], opt={"min_qual": 0})


def test_stops(way):
    """at the region's first slot with the region beginning inside the tract, at reference position 0, at an N inside the tract, and at
    the boundary of two touching regions"""
    l_ref, regions, ref, recs = TL.stop_case()
    p = check(way, TL.STOP_NAMES, l_ref, regions, ref, [b"".join(recs)], opt={"min_qual": 0})
    assert [p._place(e[0]) for e in p.events] == TL.STOP_PLACES


@pytest.mark.parametrize("max_len", (32, 31))
def test_l32(way, max_len):
    """an insertion and deletions of 32 in a period-32 repeat, a length-32 insertion that stays, an inserted N; under max_len 31 the
    events of 32 are OTHER and stay"""
    l_ref, regions, ref, recs = TL.l32_case()
    check(way, TL.L32_NAMES, l_ref, regions, ref, [b"".join(recs)], opt={"max_len": max_len, "min_qual": 0})


def test_clipping(way):
    """a read that starts inside the tract, an event behind an N op, behind a D op, behind a P op, adjacent I and D"""
    l_ref, regions, ref, recs = TL.clip_case()
    check(way, TL.CLIP_NAMES, l_ref, regions, ref, [b"".join(recs)], quality=True, opt={"min_qual": 0})


def test_wave_mix_and_a_second_add(way):
    l_ref, regions, ref, adds = TL.mix_case()
    data = [b"".join(a) for a in adds]
    want = check(way, TL.MIX_NAMES, l_ref, regions, ref, data, quality=True)
    way(True)
    got = handle(l_ref, regions, ref, data[:1], quality=True)
    first = got.indel_info()
    held = got.indel_alleles().tobytes()
    assert first["n_events"] == first["n_appended"] > 200 and first["ms_indel"] > 0
    assert held == TL.model(l_ref, regions, ref, data[:1], quality=True).indel_alleles().astype(capi.PILEUP_INDEL_ALLELE_DTYPE).tobytes()
    got.add_records(data[1])                                                    # the events held stay as they are; the new ones are aligned
    info = got.indel_info()
    assert info["n_events"] == len(want.events) and info["n_appended"] == info["n_events"] - first["n_events"] > 80
    same(got, want, TL.MIX_NAMES, THRESHOLDS[:1])
    got.close()


def test_off_is_off(way):
    """on = 0, and a handle that never made the call: byte for byte the store without rule 18"""
    mix, stop = TL.mix_case(), TL.stop_case()
    cases = [(TL.MIX_NAMES, *mix[:3], [b"".join(a) for a in mix[3]]), (TL.STOP_NAMES, *stop[:3], [b"".join(stop[3])])]
    for names, l_ref, regions, ref, data in cases:
        want = TL.model(l_ref, regions, ref, data, False, quality=True)
        moved = TL.model(l_ref, regions, ref, data, True, quality=True)
        assert want.indel_alleles().tobytes() != moved.indel_alleles().tobytes()
        for tiled in (True, False):
            way(tiled)
            for leftalign in (False, None):
                got = handle(l_ref, regions, ref, data, leftalign, quality=True)
                same(got, want, names, THRESHOLDS[:2])
                got.close()
    # the existing order of calls, the reference after the adds, is still legal on both
    way(True)
    for leftalign in (False, None):
        got = capi.Pileup(TL.C2_L_REF)
        got.set_indels()
        if leftalign is not None:
            got.set_indel_leftalign(leftalign)
        got.add_records(b"".join(TL.C2_RECS))
        got.set_ref(0, TL.C2_REF)
        assert got.indel_vcf(TL.C2_NAMES, "s1") == TL.C2_HEAD + TL.C2_OFF_ROWS[0] + TL.C2_OFF_ROWS[1]
        got.close()


def test_refusals(way):
    L = capi.lib()
    way(True)
    data = b"".join(TL.C2_RECS)
    p = capi.Pileup(TL.C2_L_REF)
    assert L.bwams_pileup_set_indel_leftalign(p.h, 1) == ERR_ARG and "indel store" in L.bwams_last_error().decode()      # no store
    assert L.bwams_pileup_set_indel_leftalign(None, 1) == ERR_ARG
    p.set_indels()
    assert L.bwams_pileup_set_indel_leftalign(p.h, 2) == ERR_ARG and L.bwams_pileup_set_indel_leftalign(p.h, -1) == ERR_ARG
    p.add_records(data)
    assert L.bwams_pileup_set_indel_leftalign(p.h, 1) == ERR_ARG and "not zero" in L.bwams_last_error().decode()         # after an add
    p.set_ref(0, TL.C2_REF)                                                     # ... on a handle without the option this stays legal
    p.close()
    # two regions, one reference set: the add is refused whole
    regions = [(0, 0, 4), (0, 4, 8)]
    p = capi.Pileup(TL.C2_L_REF, regions)
    p.set_indels()
    p.set_indel_leftalign()
    p.set_ref(0, TL.C2_REF[:4])
    n = C.c_int64(-7)
    assert L.bwams_pileup_add_records(p.h, data, len(data), C.byref(n)) == ERR_ARG and "reference" in L.bwams_last_error().decode()
    assert n.value == -7 and p.info()["n_counted"] == 0 and p.indel_info()["n_events"] == 0
    assert not any(p.fetch(k).any() or p.fetch_span(k).any() for k in range(2))
    assert L.bwams_pileup_set_indel_leftalign(p.h, 0) == 0 and L.bwams_pileup_set_indel_leftalign(p.h, 1) == 0   # still before the first add
    p.set_ref(1, TL.C2_REF[4:])
    assert p.add_records(data) == 3
    assert L.bwams_pileup_set_ref(p.h, 0, capi._p(np.ascontiguousarray(TL.C2_REF[:4]))) == ERR_ARG                # after an add
    assert "left-aligning" in L.bwams_last_error().decode()
    want = TL.model(TL.C2_L_REF, regions, [TL.C2_REF], [data])
    same(p, want, TL.C2_NAMES, THRESHOLDS[:2])
    p.reset()                                                                   # the option and the flags stay; _set_ref is legal again
    p.set_ref(0, TL.C2_REF[:4])
    assert p.add_records(data) == 3
    same(p, want, TL.C2_NAMES, THRESHOLDS[:2])
    p.reset()
    p.set_indels()                                                              # replaces the store's options: rule 18 is off again
    assert p.add_records(data) == 3
    p.set_ref(1, TL.C2_REF[4:])                                                 # and so this is legal
    same(p, TL.model(TL.C2_L_REF, regions, [TL.C2_REF], [data], None), TL.C2_NAMES, THRESHOLDS[:2])
    p.close()


def test_sorter(tmp_path):
    """a left-aligning handle on the sorted writer: a few dozen records over a homopolymer, and _vcf_all is the restatement's"""
    from test_gpu_pileup import _sorter
    rng = np.random.default_rng(41)
    g = simulate.make_genome(20000, seed=2, repeat_frac=0.0)
    ix = capi.Index.build(g, 0)
    l_ref = [400]
    text = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, 149)) + "C" + "A" * 40 + "G" + "".join("ACGT"[int(c)] for c in rng.integers(0, 4, 209))
    ref = [TL.codes(text)]
    hdr = bam.header_block(b"@HD\tVN:1.6\tSO:coordinate\n", [b"s0"], l_ref)
    recs = []
    for k in range(48):
        pos = int(rng.integers(100, 175))                                       # the read starts before or inside the tract and ends behind it
        a = 150 + int(rng.integers(max(pos - 150, 0) + 2, 38)) - pos
        cigar = ["%dM" % 100, "%dM1D%dM" % (a, 99 - a), "%dM1I%dM" % (a, 99 - a)][k % 3]
        recs.append(TL.rd(ref, 0, pos, cigar, "A" if k % 3 == 2 else "", qual=int(rng.integers(14, 41)), flag=16 * (k % 2),
                          mapq=int(rng.choice([20, 40, 60])), name=b"f%d" % k))
    runs = [b"".join(recs[0::2]), b"".join(recs[1::2])]
    try:
        p = capi.Pileup(l_ref)
        p.set_quality(min_qual=0)
        p.set_indels(min_qual=0)
        p.set_indel_leftalign()
        p.set_ref(0, ref[0])
        data0, x0, _ = _sorter(tmp_path, "plain", ix, hdr, runs)
        data1, x1, _ = _sorter(tmp_path, "leftalign", ix, hdr, runs, p=p)
        assert data0 == data1 and x0 == x1
        written = gzip.decompress(data0)[len(hdr):]
        want = pileup.Pileup(l_ref)
        want.set_quality(min_qual=0)
        want.set_indels(min_qual=0)
        want.set_indel_leftalign()
        want.set_ref(0, ref[0])
        want.add(written)
        al = want.indel_alleles()
        assert len(al) == 2 and set(al["pos"].tolist()) == {149} and int(al["n"].sum()) >= 20 and len(want.indel_calls()) == 1
        same(p, want, [b"s0"])
        p.close()
    finally:
        ix.close()
