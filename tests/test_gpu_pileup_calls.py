"""The pileup's quality plane, SNV calls and VCF text on the GPU (csrc/pileup.hip's quality sinks and pileup_call_kernel,
csrc/api_pileup.hip, host/pileup_vcf.cpp) through the C-ABI, compared exactly with bwams/pileup.py's restatement of rules 10 to 13
and with the hand-written expectations of tests/test_pileup_calls.py.  Every add runs twice, through the tiled path (both planes of a
tile in LDS) and under BWAMS_PILEUP_TILED=0 through the direct kernel alone."""
import ctypes as C
import gzip

import numpy as np
import pytest

from bwams import bam, capi, pileup, simulate
import test_pileup as T
import test_pileup_calls as TC
from test_pileup import prec

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY = -3, -4
THRESHOLDS = ((-1, -1), (0, 1), (40, 3))              # (min_qual, min_depth) of the call comparisons; -1: the handle's


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
    """both planes, and the calls and the VCF text at each pair of thresholds, against the restatement"""
    for k in range(len(want.regions)):
        assert np.array_equal(got.fetch(k), want.fetch(k)), k
        assert np.array_equal(got.fetch_quality(k), want.fetch_quality(k)), k
    for q, d in thresholds:
        w = want.calls(None if q < 0 else q, None if d < 0 else d)
        assert got.calls(q, d).tobytes() == w.astype(capi.PILEUP_CALL_DTYPE).tobytes(), (q, d)
        assert got.vcf(names, "s", q, d) == want.vcf(names, "s", None if q < 0 else q, None if d < 0 else d), (q, d)


def both(way, l_ref, regions, adds, ref, gl=None, **kw):
    """the restatement, and a device handle per route, after the same adds -> (want, tiled handle, direct handle, the infos of the
    last add)"""
    gl = gl or {}
    want = pileup.Pileup(l_ref, regions, **kw)
    want.set_quality(**gl)
    n = [want.add(d) for d in adds]
    want.set_ref_genome(ref)
    out, infos = [], []
    for tiled in (True, False):
        way(tiled)
        got = capi.Pileup(l_ref, regions, **kw)
        got.set_quality(**gl)
        assert [got.add_records(d) for d in adds] == n
        for k, (r, b, e) in enumerate(want.regions):
            got.set_ref(k, np.minimum(ref[r][b:e], 4))
        infos.append(got.info())
        assert infos[-1]["n_counted"] == n[-1] and (tiled or infos[-1]["n_entries"] == 0)
        out.append(got)
    return want, out[0], out[1], infos


def test_worked_example_and_hand_cases(way):
    want, a, b, _ = both(way, T.EX_L_REF, (), [b"".join(T.EX_RECS)], [np.array(T.EX_REF, np.uint8)])
    for got in (a, b):
        assert got.fetch_quality(0).tolist() == TC.EX_SUMS and got.calls()["pl"].tolist() == [TC.EX_PL]
        assert got.vcf(T.EX_NAMES, "s1") == TC.EX_VCF and got.text(T.EX_NAMES) == T.EX_TEXT
        same(got, want, T.EX_NAMES)
        got.close()
    want, a, b, _ = both(way, TC.HAND_L_REF, (), [b"".join(TC.HAND_RECS)], [np.array(TC.HAND_REF, np.uint8)], gl=TC.HAND_OPT, min_baseq=0)
    for got in (a, b):
        assert got.fetch_quality(0).tolist() == TC.HAND_SUMS and TC.as_tuples(got.calls()) == TC.HAND_CALLS
        assert got.vcf(TC.HAND_NAMES, "smp") == TC.HAND_VCF
        assert [int(x) for x in got.calls(min_depth=1)["pos"]] == [0, 1, 2, 4, 5, 7, 8, 9, 10]
        assert [int(x) for x in got.calls(min_qual=65)["pos"]] == [1, 2]
        same(got, want, TC.HAND_NAMES)
        got.close()


def _m(rng, pos, n, flag=0, mapq=None):
    """n random bases and qualities as nM at pos"""
    return prec(0, pos, [(n, 0)], rng.choice([1, 2, 4, 8, 15], n, p=[.24, .24, .24, .24, .04]), qual=[int(q) for q in rng.integers(0, 94, n)],
                flag=flag, mapq=int(rng.integers(0, 61)) if mapq is None else mapq)


def test_tile_and_region_edges(way):
    t = capi.Pileup([10]).info()["tile"]
    assert t == 1024
    rng = np.random.default_rng(12)
    l_ref = [2 * t + 500]                                                       # 2548 slots: the last tile is partial
    recs = []
    for edge in (t, 2 * t):                                                     # bases on slots edge - 2 .. edge + 1
        for n in (8, 33, 64, 65, 150):
            recs += [_m(rng, edge - 2, n), _m(rng, edge - n + 2, n, 16), _m(rng, edge - n // 2, n), _m(rng, edge - 1, n, 16), _m(rng, edge, n)]
    recs.append(_m(rng, t - 1, t + 2))                                          # three tiles: direct
    recs.append(_m(rng, 2 * t + 450, 120, 16))                                  # runs off the end
    ref = [rng.integers(0, 5, l_ref[0]).astype(np.uint8)]
    want, a, b, infos = both(way, l_ref, (), [b"".join(recs)], ref, min_baseq=5)
    assert infos[0]["n_slots"] == l_ref[0] and infos[0]["n_direct"] == 1 and infos[1]["n_direct"] == len(recs)
    for s in (t - 2, t - 1, t, t + 1, 2 * t - 2, 2 * t - 1, 2 * t, 2 * t + 1):
        assert want.q[s, :4].sum() > 0
    assert len(want.calls(0, 1)) > 100
    for got in (a, b):
        same(got, want, [b"one"])
        got.close()
    # regions that touch at 700, and a gap at [1500, 1600) inside records; tile edges at positions 1024 and 2148; 2800 slots
    regions = [(0, 0, 700), (0, 700, 1500), (0, 1600, 2900)]
    l_ref = [3000]
    recs = [_m(rng, 650, 100), _m(rng, 699, 2, 16), _m(rng, 1450, 150), _m(rng, 1490, 120, 16), _m(rng, 1400, 150), _m(rng, 2850, 100),
            _m(rng, 2140, 20), _m(rng, 2146, 8, 16), _m(rng, 1000, 64), prec(0, 1495, "3M2D100N2I8M", "ACGTACGTACGTA", qual=35, mapq=50)]
    ref = [rng.integers(0, 5, 3000).astype(np.uint8)]
    want, a, b, infos = both(way, l_ref, regions, [b"".join(recs)], ref, min_baseq=0)
    assert infos[0]["n_slots"] == 2800 and infos[0]["n_direct"] == 0 and infos[0]["n_entries"] > len(recs)
    assert want.fetch_quality(1, 1499, 1500).any() and want.fetch_quality(2, 1600, 1601).any() and want.fetch_quality(2, 2899, 2900).any()
    for got in (a, b):
        same(got, want, [b"one"])
        got.close()


def test_contention_and_lane_rounds(way):
    rng = np.random.default_rng(14)
    l_ref = [3000]
    # 300 records on the same 10 positions, both strands, the qualities cycling 0..93 and MAPQ 0..60: 300 additions at one slot on
    # the count and the three sums of a base, over the tile edge at 1024
    same_base = [prec(0, 1019, "10M", "ACGTACGTAC", qual=[(k + j) % 94 for j in range(10)], mapq=k % 61, flag=16 * (k & 1)) for k in range(300)]
    long_ = [_m(rng, int(rng.integers(1100, 2000)), 130, 16 * (k & 1)) for k in range(300)]      # three lane rounds each, clear of 1019
    ref = [rng.integers(0, 4, 3000).astype(np.uint8)]
    want, a, b, _ = both(way, l_ref, (), [b"".join(same_base), b"".join(long_)], ref, min_baseq=0)
    assert want.fetch(0, 1019, 1020)[0, [0, 4]].tolist() == [150, 150]
    assert int(want.fetch_quality(0, 1019, 1020)[0, 0]) == sum(min(max(min(k % 94, k % 61), 4), 60) for k in range(300))
    for got in (a, b):
        same(got, want, [b"r"])
        got.close()


def _random_input(seed: int):
    """a reference of 3000 bases with a few N, two haplotypes with planted heterozygous, hom-alt and two-ALT sites every 60 bases, and
    400 records of 30 to 150 bases read off either with errors, indels and soft clips -> (l_ref, records, reference codes, planted)"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, 3000).astype(np.uint8)
    hap = [ref.copy(), ref.copy()]
    planted = {}
    for k, x in enumerate(range(30, 2990, 60)):
        kind = ("het", "hom", "two")[k % 3]
        alt = [int(a) for a in rng.permutation([a for a in range(4) if a != ref[x]])[:2]]
        hap[0][x] = alt[0]
        hap[1][x] = {"het": ref[x], "hom": alt[0], "two": alt[1]}[kind]
        planted[x] = kind
    ref[rng.choice(3000, 20, replace=False)] = 4
    recs = []
    for k in range(400):
        n = int(rng.integers(30, 151))
        pos = int(rng.integers(0, 3000 - n))
        seq = hap[k & 1][pos:pos + n].copy()
        err = rng.random(n) < 0.02
        seq[err] = (seq[err] + rng.integers(1, 4, int(err.sum()))) % 4
        ops, codes = [], [1 << int(c) for c in seq]
        if rng.random() < 0.3:                                                  # an indel in the middle
            cut = int(rng.integers(5, n - 5))
            if rng.random() < 0.5:
                ops = [(cut, 0), (int(rng.integers(1, 4)), 2), (n - cut, 0)]
            else:
                ins = int(rng.integers(1, 4))
                ops = [(cut, 0), (ins, 1), (n - cut - ins, 0)]
        else:
            ops = [(n, 0)]
        if rng.random() < 0.3:
            clip = int(rng.integers(1, 9))
            ops, codes = [(clip, 4)] + ops, [15] * clip + codes
        if rng.random() < 0.3:
            clip = int(rng.integers(1, 9))
            ops, codes = ops + [(clip, 4)], codes + [15] * clip
        qual = None if rng.random() < 0.05 else [int(q) for q in rng.integers(2, 42, len(codes))]
        recs.append(prec(0, pos, ops, codes, qual=qual, flag=int(rng.choice([0, 16])), mapq=int(rng.choice([0, 13, 29, 60, 60, 60]))))
    return [3000], b"".join(recs), [ref], planted


@pytest.mark.parametrize("seed", [5, 6])
def test_random(way, seed):
    l_ref, data, ref, planted = _random_input(seed)
    oracle = pileup.Pileup(l_ref)
    oracle.set_quality()
    oracle.add(data)
    oracle.set_ref_genome(ref)
    calls = oracle.calls()                                                      # conditions on the input, met on the CPU alone
    kinds = {"het": 0, "hom": 0, "two": 0}
    for x in calls:
        r, a1, a2 = int(x["ref"]), int(x["a1"]), int(x["a2"])
        kind = "hom" if a1 == a2 else "het" if r in (a1, a2) else "two"
        kinds[kind] += planted.get(int(x["pos"])) == kind
    assert min(kinds.values()) >= 1, kinds
    g = oracle.genotypes()
    weak = (g["region"] >= 0) & ((g["a1"] != g["ref"]) | (g["a2"] != g["ref"])) & (g["qual"] < oracle.min_qual)
    assert weak.any() and len(oracle.calls(0, 1)) == len(calls) + int(weak.sum())
    want, a, b, infos = both(way, l_ref, (), [data], ref)
    assert infos[0]["n_entries"] > 0 and infos[1]["n_direct"] > 300
    for got in (a, b):
        same(got, want, [b"r0"])
        got.close()


def test_accumulation_and_reset(way):
    l_ref, data, ref, _ = _random_input(7)
    recs = list(bam.split_records(data))
    parts = [b"".join(recs[:150]), b"".join(recs[150:])]
    want, a, b, _ = both(way, l_ref, (), parts, ref)                            # over two adds
    whole = pileup.Pileup(l_ref)
    whole.set_quality()
    whole.add(data)
    assert np.array_equal(whole.q, want.q)
    L = capi.lib()
    for tiled, got in ((True, a), (False, b)):
        way(tiled)
        same(got, want, [b"r0"])
        assert L.bwams_pileup_set_quality(got.h, None) == ERR_ARG               # after an add, without a reset
        assert "not zero" in L.bwams_last_error().decode()
        same(got, want, [b"r0"], THRESHOLDS[:1])                                # ... and nothing was touched
        got.reset()                                                             # both planes
        assert not got.fetch(0).any() and not got.fetch_quality(0).any() and len(got.calls(0, 1)) == 0
        got.set_quality(min_qual=3, min_depth=2, no_qual_q=11)                  # directly after a reset: other options, the same plane
        assert got.add_records(parts[1]) > 0
        after = pileup.Pileup(l_ref)
        after.set_quality(min_qual=3, min_depth=2, no_qual_q=11)
        after.add(parts[1])
        after.set_ref_genome(ref)
        same(got, after, [b"r0"])
        got.close()


def test_arguments_and_capacity(way):
    L = capi.lib()
    way(True)
    p = capi.Pileup(TC.HAND_L_REF, min_baseq=0)
    n = C.c_int64(-1)
    buf = np.zeros(64, capi.PILEUP_CALL_DTYPE)
    vp = buf.ctypes.data_as(C.c_void_p)
    out = C.create_string_buffer(4096)
    assert L.bwams_pileup_fetch_quality(p.h, 0, 0, 4, vp) == ERR_ARG            # no plane yet
    assert L.bwams_pileup_calls(p.h, -1, -1, None, 0, C.byref(n)) == ERR_ARG
    assert "no quality plane" in L.bwams_last_error().decode()
    assert L.bwams_pileup_vcf(p.h, b"h\0", b"s", -1, -1, out, 4096, C.byref(n)) == ERR_ARG
    for o in (capi.PileupGlOpt(-1, 1, 30, 0), capi.PileupGlOpt(20, 0, 30, 0), capi.PileupGlOpt(20, 1, -1, 0), capi.PileupGlOpt(20, 1, 94, 0),
              capi.PileupGlOpt(20, 1, 30, 1)):
        assert L.bwams_pileup_set_quality(p.h, C.byref(o)) == ERR_ARG
    assert L.bwams_pileup_set_quality(None, None) == ERR_ARG
    assert L.bwams_pileup_fetch_quality(p.h, 0, 0, 4, vp) == ERR_ARG            # a refused call made no plane
    assert L.bwams_pileup_set_quality(p.h, None) == 0                           # NULL: {20, 1, 30, 0}
    p.set_quality(**TC.HAND_OPT)                                                # twice while the counters are zero: the options are replaced
    p.add_records(b"".join(TC.HAND_RECS))
    p.set_ref(0, TC.HAND_REF)
    assert L.bwams_pileup_calls(p.h, -1, -1, None, 0, C.byref(n)) == 0 and n.value == 5          # NULL: the count
    assert L.bwams_pileup_calls(p.h, -1, -1, vp, 4, C.byref(n)) == ERR_CAPACITY and n.value == 5
    with pytest.raises(capi.BwamsError) as e:
        p.calls(cap=4)
    assert e.value.code == ERR_CAPACITY and p.n_calls == 5 and TC.as_tuples(p.calls(cap=5)) == TC.HAND_CALLS
    assert L.bwams_pileup_calls(p.h, -1, 0, vp, 64, C.byref(n)) == ERR_ARG      # min_depth 0 is neither a depth nor "the handle's"
    assert L.bwams_pileup_calls(p.h, 1000, -1, vp, 0, C.byref(n)) == 0 and n.value == 0           # no call: nothing needed
    assert L.bwams_pileup_calls(p.h, -1, -1, vp, -1, C.byref(n)) == ERR_ARG
    assert L.bwams_pileup_vcf(p.h, b"h\0", b"smp", -1, -1, None, 0, C.byref(n)) == ERR_CAPACITY and n.value == len(TC.HAND_VCF)
    assert L.bwams_pileup_vcf(p.h, b"h\0", b"smp", -1, -1, out, len(TC.HAND_VCF) - 1, C.byref(n)) == ERR_CAPACITY
    assert L.bwams_pileup_vcf(p.h, b"h\0", b"smp", -1, -1, out, 4096, C.byref(n)) == 0 and out.raw[:n.value].decode() == TC.HAND_VCF
    assert L.bwams_pileup_vcf(p.h, None, b"smp", -1, -1, out, 4096, C.byref(n)) == ERR_ARG
    assert L.bwams_pileup_vcf(p.h, b"h\0", None, -1, -1, out, 4096, C.byref(n)) == ERR_ARG
    assert p.vcf(TC.HAND_NAMES, "smp", 1000) == TC.VCF_HEAD % ("##contig=<ID=h,length=12>\n", "smp")
    for region, beg, end in ((1, 0, 1), (-1, 0, 1), (0, 0, 13), (0, 5, 4), (0, -1, 2)):
        assert L.bwams_pileup_fetch_quality(p.h, region, beg, end, vp) == ERR_ARG, (region, beg, end)
    assert p.fetch_quality(0, 3, 3).shape == (0, 12) and p.fetch_quality(0, 2, 4).tolist() == TC.HAND_SUMS[2:4]
    p.close()


def test_unchanged_without_and_with_the_plane(way):
    l_ref, data, ref, _ = _random_input(8)
    for tiled in (True, False):
        way(tiled)
        plain, with_q = capi.Pileup(l_ref), capi.Pileup(l_ref)
        with_q.set_quality()
        assert plain.add_records(data) == with_q.add_records(data)
        for h in (plain, with_q):
            h.set_ref(0, ref[0])
        assert np.array_equal(plain.fetch(0), with_q.fetch(0)) and plain.fetch(0).any()
        for pair in ((2, 200), (1, 0)):
            assert plain.sites(*pair).tobytes() == with_q.sites(*pair).tobytes() and len(plain.sites(*pair)) > 5
            assert plain.text([b"r0"], *pair) == with_q.text([b"r0"], *pair)
        i, j = plain.info(), with_q.info()
        assert all(i[k] == j[k] for k in ("tile", "n_slots", "n_counted", "n_entries", "n_direct"))
        plain.close(); with_q.close()


def test_sorter(tmp_path):
    """a quality-enabled handle set on a sorted writer that marks duplicates: the sums and calls of the records as written, and the
    file and its index byte for byte those of a sorter without the handle"""
    from test_gpu_pileup import _sorter
    rng = np.random.default_rng(23)
    g = simulate.make_genome(20000, seed=2, repeat_frac=0.0)
    ix = capi.Index.build(g, 0)
    l_ref = [1500]
    hdr = bam.header_block(b"@HD\tVN:1.6\tSO:coordinate\n", [b"s0"], l_ref)
    ref = rng.integers(0, 4, 1500).astype(np.uint8)
    recs = []
    for k in range(60):
        pos = int(rng.integers(0, 1400))
        seq = ref[pos:pos + 80].copy()
        seq[::7] = (seq[::7] + 1 + k % 2) % 4                                   # every seventh base off the reference, two ways
        recs.append(prec(0, pos, "80M", [1 << int(c) for c in seq], qual=[int(q) for q in rng.integers(5, 41, 80)], flag=16 * (k % 2),
                         mapq=int(rng.choice([20, 40, 60])), name=b"f%d" % k))
    dup = prec(0, 700, "80M", [1 << int(c) for c in ref[700:780]], qual=40, name=b"d0")
    recs += [dup, prec(0, 700, "80M", [1, 2, 4, 8] * 20, qual=20, name=b"d1")]   # the second is the duplicate of the first: it drops out
    runs = [b"".join(recs[0::2]), b"".join(recs[1::2])]
    try:
        p = capi.Pileup(l_ref)
        p.set_quality(min_qual=0)
        data0, x0, _ = _sorter(tmp_path, "plain", ix, hdr, runs)
        data1, x1, st = _sorter(tmp_path, "calls", ix, hdr, runs, p=p)
        assert data0 == data1 and x0 == x1
        p.set_ref(0, ref)
        written = gzip.decompress(data0)[len(hdr):]
        want = pileup.Pileup(l_ref)
        want.set_quality(min_qual=0)
        assert want.add(written) == st.records - st.dup.records_marked == len(recs) - 1 and st.dup.records_marked == 1
        want.set_ref(0, ref)
        assert len(want.calls()) > 20
        same(p, want, [b"s0"])
        asgiven = pileup.Pileup(l_ref)                                          # with the duplicate the sums differ
        asgiven.set_quality(min_qual=0)
        asgiven.add(b"".join(runs))
        assert not np.array_equal(asgiven.fetch_quality(0, 700, 780), want.fetch_quality(0, 700, 780))
        p.close()
    finally:
        ix.close()
