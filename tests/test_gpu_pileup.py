"""Pileup on the GPU (csrc/pileup.hip, csrc/api_pileup.hip, host/bam_sort.cpp's bwams_sorter_set_pileup) through the C-ABI, compared
exactly with bwams/pileup.py's restatement of the rules and with the hand-written expectations of tests/test_pileup.py.  Every add
runs twice, through the tiled path and under BWAMS_PILEUP_TILED=0 through the direct kernel alone."""
import ctypes as C
import gzip

import numpy as np
import pytest

from bwams import bam, capi, pileup, simulate
import test_pileup as T
from test_depth import rec
from test_pileup import ch, prec

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY = -3, -4
PIECE = 256 * 65280                                   # the sorter's deflate piece
PAIRS = ((2, 200), (1, 0), (3, 500))                  # (min_alt, min_permille) of the site comparisons


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


@pytest.fixture
def way(monkeypatch):
    """way(tiled): the route of the adds that follow (BWAMS_PILEUP_TILED through bwams_debug_reload); the default again afterwards"""
    def set_(tiled: bool):
        monkeypatch.setenv("BWAMS_PILEUP_TILED", "1" if tiled else "0")
        capi.debug_reload()
    yield set_
    monkeypatch.undo()
    capi.debug_reload()


def same(got: capi.Pileup, want: pileup.Pileup, names=None, pairs=PAIRS):
    """every counter, and the sites and the text at each pair of thresholds, against the restatement"""
    for k in range(len(want.regions)):
        assert np.array_equal(got.fetch(k), want.fetch(k)), k
    for a, m in pairs:
        s, w = got.sites(a, m), want.sites(a, m)
        assert s.tobytes() == w.astype(capi.PILEUP_SITE_DTYPE).tobytes(), (a, m)
        if names is not None:
            assert got.text(names, a, m) == want.text(names, a, m), (a, m)


def both(way, l_ref, regions, adds, ref=None, **kw):
    """the restatement, and a device handle per route, after the same adds -> (want, tiled handle, direct handle, the infos of the
    last add)"""
    want = pileup.Pileup(l_ref, regions, **kw)
    n = [want.add(d) for d in adds]
    if ref is not None:
        want.set_ref_genome(ref)
    out, infos = [], []
    for tiled in (True, False):
        way(tiled)
        got = capi.Pileup(l_ref, regions, **kw)
        assert [got.add_records(d) for d in adds] == n
        if ref is not None:
            for k, (r, b, e) in enumerate(want.regions):
                got.set_ref(k, np.minimum(ref[r][b:e], 4))
        infos.append(got.info())
        assert infos[-1]["n_counted"] == n[-1] and (tiled or infos[-1]["n_entries"] == 0)
        out.append(got)
    return want, out[0], out[1], infos


def test_hand_records(way, toy):
    data = b"".join(T.HAND)
    ref = [T.REF0, np.array([4, 1, 4, 4, 4, 4], np.uint8)]
    want, a, b, infos = both(way, T.L_REF, T.REGIONS, [data], ref=ref, min_alt=1, min_permille=300)
    for got in (a, b):
        assert [got.fetch(k).tolist() for k in range(3)] == T.WANT
        same(got, want, T.NAMES)
        assert got.text(T.NAMES).startswith(T.HAND_TEXT)
        assert [int(x) for x in got.sites(2, 0)["pos"]] == [5, 15]
    assert infos[0]["n_counted"] == T.N_COUNTED and infos[0]["n_direct"] == 0 and infos[1]["n_direct"] == 14     # 2 of the 16 reach no slot
    L = capi.lib()
    n = C.c_int64(7)
    for got in (a, b):                                                          # rule 3's two refusals: nothing of the call is added
        bad = prec(0, 2, "3M", "CCC") * 70 + prec(-1, 0, [(2, 0), (1, 9)], "CC", flag=0x4) + prec(0, 0, [(1, 12)], "C")
        assert L.bwams_pileup_add_records(got.h, bad, len(bad), C.byref(n)) == ERR_ARG
        assert L.bwams_last_error().decode() == "bwams_pileup_add_records: record 70 has a CIGAR op code above 8"
        bad = prec(0, 2, "3M", "CCC") * 65 + prec(0, 0, "2M", "CCC", flag=0x400) + prec(0, 0, "2M1I", "CC") + prec(0, 0, "2M", "CCC")
        assert L.bwams_pileup_add_records(got.h, bad, len(bad), C.byref(n)) == ERR_ARG
        assert L.bwams_last_error().decode() == "bwams_pileup_add_records: record 66 has a CIGAR whose query length is not l_seq"
        assert [got.fetch(k).tolist() for k in range(3)] == T.WANT
        cut = prec(0, 0, "5M", "ACGTA")
        assert L.bwams_pileup_add_records(got.h, cut[:-1], len(cut) - 1, None) == ERR_ARG     # the chain, as bwams_bam_upload checks it
        short = bytearray(prec(0, 0, "9M", "ACGTACGTA")[:-3])                                 # QUAL ends behind the record
        short[0:4] = (len(short) - 4).to_bytes(4, "little")
        assert L.bwams_pileup_add_records(got.h, bytes(short), len(short), None) == ERR_ARG
        assert L.bwams_last_error().decode() == "bwams_pileup_add_records: record 0 ends inside its SEQ or QUAL"
        got.reset()
        assert not got.fetch(0).any() and len(got.sites()) == 0
    for tiled in (True, False):                                                 # I behind S, I behind D, two I around a P at one anchor
        way(tiled)
        ins = capi.Pileup([10])
        assert ins.add_records(b"".join(T.INS_RECS)) == 3 and ins.fetch(0, 4, 7).tolist() == T.INS_WANT and not ins.fetch(0, 0, 4).any()
        ins.close()
    ex = capi.Pileup(T.EX_L_REF)                                                # the header's worked example
    assert ex.add_records(b"".join(T.EX_RECS)) == 7
    ex.set_ref(0, T.EX_REF)
    assert ex.text(T.EX_NAMES) == T.EX_TEXT
    bt = capi.Batch(toy[1], 1000, 1000 * 160)                                   # the same records from a batch, in HBM
    try:
        assert bt.bam_upload(data) == len(T.HAND)
        way(True)
        assert a.add_batch(bt) == T.N_COUNTED and [a.fetch(k).tolist() for k in range(3)] == T.WANT
    finally:
        bt.close()
    for got in (a, b, ex):
        got.close()


def test_tile_and_region_edges(way):
    t = capi.Pileup([10]).info()["tile"]
    assert t >= 1024
    rng = np.random.default_rng(2)

    def m(pos, n, flag=0):
        return prec(0, pos, [(n, 0)], rng.choice([1, 2, 4, 8, 15], n), qual=[int(q) for q in rng.integers(10, 40, n)], flag=flag)

    l_ref = [5 * t + 100]
    recs = [m(t - 50, 50),                                                      # ends at slot T - 1: one tile
            m(t, 50, 16),                                                       # starts at slot T: one tile
            m(t - 25, 50),                                                      # straddles T - 1 | T: two tiles
            m(2 * t - 1, 2, 16),                                                # one base on either side
            m(t, t),                                                            # a whole tile and no more
            m(t - 1, t + 1),                                                    # exactly two tiles, to the first's last slot ...
            m(t - 1, t + 2),                                                    # ... and one more base: three tiles, direct
            prec(0, 3 * t - 5, [(10, 0), (t, 3), (10, 0)], "ACGTACGTACACGTACGTAC"),           # an N skip over a whole tile: direct
            prec(0, 2 * t, [(0, 0), (2, 1), (3, 0)], "TTACG"),                  # an I behind a reference op of length 0: its anchor is slot 2T - 1
            m(5 * t + 90, 30),                                                  # runs off the end, in the last and partial tile
            m(5 * t + 100, 5)]                                                  # POS at the end: no slot
    want, a, b, infos = both(way, l_ref, (), [b"".join(recs)], ref=[rng.integers(0, 5, l_ref[0]).astype(np.uint8)])
    assert infos[0]["n_slots"] == l_ref[0] and infos[0]["n_direct"] == 2 and infos[0]["n_entries"] == 1 + 1 + 2 + 2 + 1 + 2 + 2 + 1
    assert infos[1]["n_direct"] == 10
    assert a.fetch(0, 2 * t - 1, 2 * t)[0, pileup.INS] == 1
    assert not want.c[3 * t + 5:4 * t - 5].any() and want.c[4 * t + 5:4 * t + 15, :8].sum() == 10               # tile 3 all but empty
    for got in (a, b):
        same(got, want, [b"one"])
        got.close()
    # a region of one position; two touching regions; a gap that a record spans; region edges inside a tile; the last region ends its tile early
    regions = [(0, 10, 11), (0, 100, 600), (0, 600, 900), (0, 1000, 1000 + t + 200), (1, 0, 1), (1, 7, 8)]
    l_ref = [5 * t + 100, 8]
    recs = [m(5, 10), m(10, 1), m(0, 120), m(550, 100, 16), m(850, 200), m(880, 40), m(990 + t, 300), m(1150 + t, 100),
            prec(0, 895, "3M4D100N3M", "ACGTAC"), prec(1, 0, "8M", "ACGTACGT"), prec(1, 6, "1M1I1M", "ACG", flag=16)]
    ref = [rng.integers(0, 5, n).astype(np.uint8) for n in l_ref]
    want, a, b, infos = both(way, l_ref, regions, [b"".join(recs)], ref=ref)
    assert infos[0]["n_slots"] == 1 + 500 + 300 + t + 200 + 2 and infos[0]["n_direct"] == 0
    assert a.fetch(0).tolist() == want.fetch(0).tolist() != [[0] * 12] and a.fetch(5, 7, 8)[0, pileup.INS] == 0 and a.fetch(5)[0, :8].sum() == 2
    for got in (a, b):
        same(got, want, [b"one", b"two"])
        got.close()
    # occupied tiles with empty tiles between them, twice: the second add comes on top; then no record and one
    far = [m(3, 20), m(4 * t + 7, 20, 16)]
    want, a, b, infos = both(way, [5 * t + 100], (), [b"".join(far), b"", b"".join(far[1:])])
    assert infos[0]["n_entries"] == 1 and infos[0]["n_counted"] == 1
    empty = capi.Pileup([5 * t + 100])
    assert empty.add_records(b"") == 0 and empty.info()["n_entries"] == 0 and not empty.fetch(0, 0, 50).any()
    for got in (a, b):
        same(got, want)
        got.close()
    empty.close()


def test_lane_rounds_and_contention(way):
    rng = np.random.default_rng(4)
    l_ref = [3000]
    recs = []
    for n in (64, 65, 128, 129, 1, 63):                                         # the lanes' rounds of 64 bases
        recs.append(prec(0, int(rng.integers(0, 2000)), [(n, 0)], rng.choice([1, 2, 4, 8], n), qual=[int(q) for q in rng.integers(0, 41, n)],
                         flag=16 * (n & 1)))
    ops = [(1, 4)] + [(int(rng.integers(1, 4)), op) for _ in range(17) for op in (0, 1, 0, 2)] + [(2, 0)]      # 70 ops: S, 17 x (M I M D), M
    l_seq = sum(n for n, op in ops if op in (0, 1, 4))
    assert len(ops) == 70
    recs.append(prec(0, 700, ops, rng.choice([1, 2, 4, 8, 15], l_seq), qual=[int(q) for q in rng.integers(0, 41, l_seq)]))
    recs.append(prec(0, 900, "5M200D5M", "ACGTAACGTA"))                         # a D of several lane steps, over the tile edge at 1024
    ops = [(1, 0), (1, 1)] * 100                                                # 200 ops: the op rounds' carry
    recs.append(prec(0, 1500, ops, rng.choice([1, 2, 4, 8], 200)))
    want, a, b, _ = both(way, l_ref, (), [b"".join(recs)], ref=[rng.integers(0, 4, 3000).astype(np.uint8)])
    assert want.fetch(0, 1500, 1600)[:, pileup.INS].tolist() == [1] * 100 and want.fetch(0, 905, 1105)[:, pileup.DEL].min() == 1
    for got in (a, b):
        same(got, want, [b"r"])
        got.close()
    pile = prec(0, 1023, "2M", "AC") * 300                                      # 300 on one address; then again: the flush adds to what is there
    want, a, b, _ = both(way, l_ref, (), [pile, pile])
    for got in (a, b):
        assert got.fetch(0, 1022, 1026).tolist() == [ch(), [600] + [0] * 11, [0, 600] + [0] * 10, ch()]
        same(got, want)
        got.close()


def _random_cigar(rng, n_ops):
    """every op; S and H only at the ends, as SAM has them; ops of length 0 among them (tests/test_gpu_depth.py's generator)"""
    ops = []
    if rng.random() < 0.3:
        ops.append((int(rng.integers(1, 9)), 5))
    if rng.random() < 0.4:
        ops.append((int(rng.integers(1, 9)), 4))
    for _ in range(n_ops):
        ops.append((int(rng.integers(0, 12)), int(rng.choice([0, 0, 0, 1, 2, 3, 6, 7, 8]))))
    if rng.random() < 0.4:
        ops.append((int(rng.integers(1, 9)), 4))
    if rng.random() < 0.3:
        ops.append((int(rng.integers(1, 9)), 5))
    return ops


def _random_record(rng, l_ref, ops=None):
    ops = _random_cigar(rng, int(rng.integers(1, 12))) if ops is None else ops
    l_seq = sum(n for n, op in ops if op in (0, 1, 4, 7, 8))
    r = int(rng.integers(0, len(l_ref)))
    qual = None if rng.random() < 0.1 else [int(q) for q in rng.integers(0, 41, l_seq)]
    return prec(r, int(rng.integers(-1, l_ref[r] + 20)), ops, rng.integers(0, 16, l_seq), qual=qual, flag=int(rng.choice([0, 16, 16 | 1, 0x400])),
                mapq=int(rng.integers(0, 61)))


@pytest.fixture(scope="module")
def random_case():
    rng = np.random.default_rng(17)
    l_ref = [3001, 2500]
    recs = [_random_record(rng, l_ref) for _ in range(2000)]
    recs += [_random_record(rng, l_ref, [(40, 0), (int(rng.integers(900, 2100)), 3), (40, 0)]) for _ in range(10)]      # N skips and long
    recs += [_random_record(rng, l_ref, [(int(rng.integers(1100, 2300)), 0)]) for _ in range(10)]                      # reads: direct
    recs.append(prec(0, 10, "2990M", rng.integers(0, 16, 2990), qual=[int(q) for q in rng.integers(0, 41, 2990)]))     # more than two tiles of "few" too
    ref = [rng.integers(0, 5, n).astype(np.uint8) for n in l_ref]
    ones = [(0, int(x)) for x in np.sort(rng.choice(3001, 2300, replace=False))] + \
           [(1, int(x)) for x in np.sort(rng.choice(2500, 300, replace=False))]                                         # 2600 slots: three tiles
    lists = {"all": (), "few": [(0, 17, 900), (0, 900, 1100), (0, 2000, 3001), (1, 1, 2), (1, 1200, 2500)],
             "ones": [(r, x, x + 1) for r, x in ones]}
    return l_ref, b"".join(recs), ref, lists


@pytest.mark.parametrize("which", ["all", "few", "ones"])
def test_random(way, random_case, which):
    l_ref, data, ref, lists = random_case
    want, a, b, infos = both(way, l_ref, lists[which], [data], ref=ref, min_mapq=5)
    assert want.c.sum() > 1000 and all(len(want.sites(*p)) > 5 for p in PAIRS[:2])
    assert infos[0]["n_entries"] > 0 and infos[1]["n_direct"] > infos[0]["n_direct"]
    assert infos[0]["n_direct"] >= 1                                            # both routes ran
    for got in (a, b):
        same(got, want, [b"r0", b"r1"])
        got.close()


def test_reference(way):
    rng = np.random.default_rng(8)
    seqs = ["".join(rng.choice(list("ACGT"), 700)), "".join(rng.choice(list("ACGT"), 90))]
    seqs[0] = seqs[0][:300] + "N" * 25 + seqs[0][325:640] + "NRY" + seqs[0][643:]
    fasta = ">a first\n" + "\n".join(seqs[0][k:k + 60] for k in range(0, 700, 60)) + "\n>b\n" + seqs[1] + "\n"
    codes = [np.array(["ACGT".find(c) if c in "ACGT" else 4 for c in s], np.uint8) for s in seqs]
    l_ref = [700, 90]
    regions = [(0, 250, 400), (0, 630, 700), (1, 0, 90)]
    recs = [prec(0, int(p), "50M", rng.choice([1, 2, 4, 8], 50)) for p in rng.integers(200, 650, 300)]
    recs += [prec(1, int(p), "30M", rng.choice([1, 2, 4, 8], 30), flag=16) for p in rng.integers(0, 60, 60)]
    want, a, b, _ = both(way, l_ref, regions, [b"".join(recs)], ref=codes, min_alt=1, min_permille=0)
    assert int(want.c[50:75, :8].sum()) > 0 and not np.isin(want.sites()["pos"][want.sites()["region"] == 0], np.arange(300, 325)).any()
    ix = capi.Index.from_fasta(fasta.encode())
    try:
        for got in (a, b):
            same(got, want, [b"a", b"b"])                                       # from host codes
            got.set_ref(0, np.full(150, 4, np.uint8))
            assert not (got.sites()["region"] == 0).any()
            got.set_ref_index(ix)                                               # gathered from the index: the N run reads 4
            same(got, want, [b"a", b"b"])
        L = capi.lib()
        assert L.bwams_pileup_set_ref(a.h, 3, codes[0].ctypes.data_as(C.c_void_p)) == ERR_ARG
        assert L.bwams_pileup_set_ref(a.h, 0, np.full(150, 5, np.uint8).ctypes.data_as(C.c_void_p)) == ERR_ARG
        other = capi.Pileup([700, 91])
        assert L.bwams_pileup_set_ref_index(other.h, ix.h) == ERR_ARG          # lengths that are not the index's
        other.close()
        other = capi.Pileup([700])
        assert L.bwams_pileup_set_ref_index(other.h, ix.h) == ERR_ARG          # another number of references
        assert L.bwams_pileup_set_ref_index(other.h, None) == ERR_ARG
        g = simulate.make_genome(3000, seed=3, repeat_frac=0.0)
        bare = capi.Index.build(g, 0)                                           # no contigs
        assert L.bwams_pileup_set_ref_index(other.h, bare.h) == ERR_ARG
        bare.close()
        other.close()
    finally:
        ix.close()
    for got in (a, b):
        got.close()


def test_from_a_real_batch(way, toy):
    from test_gpu_markdup import _pe_chunk
    g, ix = toy
    rng = np.random.default_rng(5)
    l_ref = [150000, len(g) - 150000]
    sample = g.copy()
    at = rng.choice(len(g), 400, replace=False)
    sample[at] = (g[at] + rng.integers(1, 4, 400)) % 4                          # planted SNVs: the reads come from `sample`
    t1, t2, _ = _pe_chunk(sample, 1200, 8)
    b = capi.Batch(ix, 4000, 4000 * 160)
    try:
        b.process_chunk2(t1, t2)
        b.bam_run()
        raw, _ = b.bam_fetch()
        want = pileup.Pileup(l_ref)
        n = want.add(raw)
        want.set_ref_genome([g[:150000], g[150000:]])
        for tiled in (True, False):
            way(tiled)
            got = capi.Pileup(l_ref)
            assert got.add_batch(b) == n > 2000
            got.set_ref_index(ix)                                               # an index without .amb: its bases as they are
            same(got, want, pairs=PAIRS[:2])
            got.close()
        hit = np.isin(want.sites()["pos"] + np.array([0, 150000])[want.sites()["region"]], at)
        assert hit.sum() > 20                                                   # planted positions among the sites (no threshold on recall)
    finally:
        b.close()


def _fragment(k: int, refid: int, pos: int, flag: int = 0, qual: int = 40, pad: int = 0) -> bytes:
    return rec(refid, pos, "100M", flag=flag, name=b"f%d" % k, qual=qual, pad=pad)          # SEQ: 100 A


def _sorter(tmp_path, tag, ix, hdr, runs, p=None, d=None, markdup=True):
    path = str(tmp_path / ("%s.bam" % tag))
    s = capi.Sorter(path, 0, hdr, markdup=markdup)
    b = capi.Batch(ix, 1000, 1000 * 160)
    try:
        if p is not None:
            s.set_pileup(p)
        if d is not None:
            s.set_depth(d)
        for k, run in enumerate(runs):
            b.bam_upload(run)
            s.put_batch(k, b)
            if k == 0 and p is not None:
                assert capi.lib().bwams_sorter_set_pileup(s.h, p.h) == ERR_ARG  # after a put
    finally:
        st = s.close()
        b.close()
    return open(path, "rb").read(), open(path + ".bai", "rb").read(), st


def test_sorter(tmp_path, toy):
    _, ix = toy
    rng = np.random.default_rng(21)
    l_ref = [5000, 3000]
    hdr = bam.header_block(b"@HD\tVN:1.6\tSO:coordinate\n", [b"s0", b"s1"], l_ref)
    runs, k = [], 0
    for put in range(3):
        recs = []
        for _ in range(800):
            recs.append(_fragment(k, int(rng.integers(0, 2)), int(rng.integers(0, 2800)), flag=16 * int(rng.integers(0, 2))))
            k += 1
        runs.append(recs)
    runs[0].insert(5, _fragment(90000, 0, 4000, qual=40))                       # kept: the best of its place ...
    runs[2].insert(9, _fragment(90001, 0, 4000, qual=20))                       # ... its duplicate comes two puts later
    runs[1].insert(3, _fragment(90002, 1, 2990, flag=0x400))                    # a stale mark on a record that is no duplicate: cleared
    runs = [b"".join(r) for r in runs]
    regions = [(0, 100, 4500), (1, 0, 3000)]
    p1, p2, d2, d3 = capi.Pileup(l_ref, regions), capi.Pileup(l_ref, regions), capi.Depth(l_ref), capi.Depth(l_ref)
    data0, x0, st0 = _sorter(tmp_path, "plain", ix, hdr, runs)
    data1, x1, st1 = _sorter(tmp_path, "pileup", ix, hdr, runs, p=p1)
    data2, x2, st2 = _sorter(tmp_path, "both", ix, hdr, runs, p=p2, d=d2)
    data3, x3, _ = _sorter(tmp_path, "depth", ix, hdr, runs, d=d3)
    assert data0 == data1 == data2 == data3 and x0 == x1 == x2 == x3            # the file and its index do not know about the handles
    written = gzip.decompress(data0)[len(hdr):]
    want = pileup.Pileup(l_ref, regions)
    n = want.add(written)
    assert st1.dup.records_marked >= 1 and n == st1.records - st1.dup.records_marked
    for p in (p1, p2):
        same(p, want)
        assert p.fetch(0, 4000, 4001)[0].tolist() == ch("A+") and p.fetch(1, 2995, 2996)[0].tolist() == ch("A+")      # one of the two; the stale mark gone
    asgiven = pileup.Pileup(l_ref, regions)
    asgiven.add(b"".join(runs))
    assert asgiven.fetch(0, 4000, 4001)[0].tolist() == [2] + [0] * 11 and not asgiven.fetch(1, 2995, 2996).any()
    d2.finish(); d3.finish()
    assert all(np.array_equal(d2.fetch(r), d3.fetch(r)) for r in range(2))      # the depth is what it is without the pileup handle
    assert np.array_equal(d2.fetch(1), p2.fetch(1)[:, :8].sum(1))
    L = capi.lib()
    s = capi.Sorter(str(tmp_path / "args.bam"), 0, hdr)
    other = capi.Pileup([5000, 3001])
    assert L.bwams_sorter_set_pileup(s.h, other.h) == ERR_ARG                   # lengths that are not the header's
    assert L.bwams_last_error().decode() == "bwams_sorter_set_pileup: the pileup handle's reference lengths are not the sorter header's"
    assert L.bwams_sorter_set_pileup(s.h, None) == ERR_ARG
    n_dev = C.c_int(0)
    L.bwams_device_count(C.byref(n_dev))
    if n_dev.value > 1:                                                         # with one GPU this case does not run
        far = capi.Pileup(l_ref, device=1)
        assert L.bwams_sorter_set_pileup(s.h, far.h) == ERR_ARG                 # another device
        far.close()
    s.close()
    for h in (p1, p2, d2, d3, other):
        h.close()


def test_sorter_record_across_pieces(tmp_path, toy):
    """just over one deflate piece of records: one straddles the cut and is counted once, with the flag the merge gave it.  Every
    record is 100M of A on the forward strand, so A+ is the depth, which numpy gives in closed form."""
    _, ix = toy
    rng = np.random.default_rng(33)
    l_ref = [200000]
    hdr = bam.header_block(b"@HD\tVN:1.6\tSO:coordinate\n", [b"big"], l_ref)
    n = 60000
    pos = np.sort(rng.choice(199000, n, replace=False))                         # distinct places: no duplicates, every stale mark cleared
    recs = [_fragment(k, 0, int(x), flag=0x400 if k % 3 == 0 else 0, qual=30, pad=int(rng.integers(80, 120))) for k, x in enumerate(pos)]
    size = np.cumsum([0] + [len(r) for r in recs])
    assert size[-1] > PIECE and ((size[:-1] < PIECE) & (size[1:] > PIECE)).any()                 # a straddler at the cut
    runs = [b"".join(recs[k::3]) for k in range(3)]                             # the merge interleaves them back into `recs`
    diff = np.zeros(l_ref[0] + 1, np.int64)
    np.add.at(diff, pos, 1)
    np.add.at(diff, pos + 100, -1)
    for tag, with_depth in (("cut", False), ("cut_both", True)):                # a pileup handle alone, then beside a depth handle
        p, d = capi.Pileup(l_ref), capi.Depth(l_ref) if with_depth else None
        data, _, st = _sorter(tmp_path, tag, ix, hdr, runs, p=p, d=d)
        assert st.records == n and st.dup.records_marked == 0
        c = p.fetch(0)
        assert np.array_equal(c[:, 0], np.cumsum(diff)[:-1]) and not c[:, 1:].any() and int(c[:, 0].sum()) == 100 * n
        p.close()
        if d is not None:
            assert np.array_equal(d.finish().fetch(0), c[:, 0])
            d.close()


def test_capacity_and_arguments(way):
    L = capi.lib()
    way(True)
    p = capi.Pileup(T.EX_L_REF)
    p.add_records(b"".join(T.EX_RECS))
    p.set_ref(0, T.EX_REF)
    n = C.c_int64(0)
    buf = np.zeros(64, capi.PILEUP_SITE_DTYPE)
    vp = buf.ctypes.data_as(C.c_void_p)
    assert L.bwams_pileup_sites(p.h, -1, -1, None, 0, C.byref(n)) == 0 and n.value == 3       # NULL: the count
    assert L.bwams_pileup_sites(p.h, -1, -1, vp, 2, C.byref(n)) == ERR_CAPACITY and n.value == 3
    with pytest.raises(capi.BwamsError) as e:
        p.sites(cap=2)
    assert e.value.code == ERR_CAPACITY and p.n_sites == 3 and len(p.sites(cap=3)) == 3
    assert L.bwams_pileup_sites(p.h, 0, -1, vp, 64, C.byref(n)) == ERR_ARG and L.bwams_pileup_sites(p.h, -1, 1001, vp, 64, C.byref(n)) == ERR_ARG
    assert L.bwams_pileup_sites(p.h, 100, -1, vp, 0, C.byref(n)) == 0 and n.value == 0        # no site: nothing needed
    out = C.create_string_buffer(1024)
    assert L.bwams_pileup_text(p.h, b"c1\0", -1, -1, None, 0, C.byref(n)) == ERR_CAPACITY and n.value == len(T.EX_TEXT)
    assert L.bwams_pileup_text(p.h, b"c1\0", -1, -1, out, len(T.EX_TEXT) - 1, C.byref(n)) == ERR_CAPACITY
    assert L.bwams_pileup_text(p.h, b"c1\0", -1, -1, out, 1024, C.byref(n)) == 0 and out.raw[:n.value].decode() == T.EX_TEXT
    assert L.bwams_pileup_text(p.h, None, -1, -1, out, 1024, C.byref(n)) == ERR_ARG
    for region, beg, end in ((1, 0, 1), (-1, 0, 1), (0, 0, 9), (0, 5, 4), (0, -1, 2)):
        assert L.bwams_pileup_fetch(p.h, region, beg, end, vp) == ERR_ARG, (region, beg, end)
    assert p.fetch(0, 3, 3).shape == (0, 12) and p.fetch(0, 7, 8).tolist() == [ch("T+", "T+", "T-", "T+", "T+")]
    q = capi.Pileup([30], [(0, 10, 20)])
    assert L.bwams_pileup_fetch(q.h, 0, 9, 12, vp) == ERR_ARG and L.bwams_pileup_fetch(q.h, 0, 12, 21, vp) == ERR_ARG
    assert q.info()["n_slots"] == 10 and q.info()["n_regions"] == 1 and capi.Pileup([30, 0, 4]).info()["n_regions"] == 2
    q.close()
    p.close()
    h = C.c_void_p()
    l_ref = np.array([10, 20], np.int32)
    for bad in ([(0, 0, 5), (0, 4, 8)], [(0, 5, 8), (0, 0, 5)], [(1, 0, 5), (0, 0, 5)], [(0, 0, 11)], [(0, 5, 5)], [(0, -1, 5)], [(2, 0, 1)]):
        reg = np.array(bad, np.int32)
        assert L.bwams_pileup_open(0, l_ref.ctypes.data_as(C.c_void_p), 2, reg.ctypes.data_as(C.c_void_p), len(bad), None, C.byref(h)) == ERR_ARG, bad
    ok = np.array([(0, 0, 5), (0, 5, 10), (1, 19, 20)], np.int32)                # touching regions are allowed
    assert L.bwams_pileup_open(0, l_ref.ctypes.data_as(C.c_void_p), 2, ok.ctypes.data_as(C.c_void_p), 3, None, C.byref(h)) == 0
    assert L.bwams_pileup_close(h) == 0 and L.bwams_pileup_close(None) == 0
    for o in (capi.PileupOpt(0x10000, 0, 13, 2, 200, 0), capi.PileupOpt(0x704, 0, 256, 2, 200, 0), capi.PileupOpt(0x704, 0, 13, 0, 200, 0),
              capi.PileupOpt(0x704, 0, 13, 2, 1001, 0), capi.PileupOpt(0x704, 0, 13, 2, 200, 1)):
        assert L.bwams_pileup_open(0, l_ref.ctypes.data_as(C.c_void_p), 2, None, 0, C.byref(o), C.byref(h)) == ERR_ARG
