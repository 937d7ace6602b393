"""Alignment QC on the GPU (csrc/qc.hip, csrc/api_qc.hip, host/bam_sort.cpp's bwams_sorter_set_qc) through the C-ABI, compared exactly
with bwams/qc.py's restatement of the rules and with the hand-written expectations of tests/test_qc.py.  Every add runs twice,
through the lane-per-cycle kernel and under BWAMS_QC_LANES=0 through the plain kernel; every comparison covers the summary, all six
tables and both texts."""
import ctypes as C
import gzip

import numpy as np
import pytest

from bwams import bam, capi, qc, simulate
import test_qc as T
from test_depth import rec
from test_qc import aux_int, qrec

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY = -3, -4
PIECE = 256 * 65280                                   # the sorter's deflate piece


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
    """way(lanes): the kernel of the adds that follow (BWAMS_QC_LANES through bwams_debug_reload); the default again afterwards"""
    def set_(lanes: bool):
        monkeypatch.setenv("BWAMS_QC_LANES", "1" if lanes else "0")
        capi.debug_reload()
    yield set_
    monkeypatch.undo()
    capi.debug_reload()


def same(got: capi.Qc, want: qc.Qc):
    """the summary, all six tables and both texts against the restatement"""
    flags, scalars = got.summary()
    assert flags.tolist() == want.flags.tolist()
    assert scalars.tolist() == want.scalars.tolist()
    for what in range(6):
        g, w = got.table(what), want.table(what)
        assert g.shape == w.shape and np.array_equal(g, w), (what, np.flatnonzero(g != w)[:8])
    for what in (qc.TEXT_FLAGSTAT, qc.TEXT_STATS):
        assert got.text(what) == want.text(what), what


def both(way, adds, **opt):
    """the restatement, and a device handle per kernel, after the same adds -> (want, lanes handle, plain handle)"""
    want = qc.Qc(**opt)
    n = [want.add(d) for d in adds]
    out = []
    for lanes in (True, False):
        way(lanes)
        got = capi.Qc(**opt)
        assert [got.add_records(d) for d in adds] == n
        i = got.info()
        assert i["n_counted"] == n[-1] and i["n_records"] == len(bam.split_records(adds[-1]))
        same(got, want)
        out.append(got)
    return want, out[0], out[1]


def test_hand_records(way, toy):
    data = b"".join(T.HAND)
    want, a, b = both(way, [data], **T.HAND_OPT)
    for got in (a, b):
        flags, scalars = got.summary()
        assert flags.tolist() == T.HAND_FLAGS
        assert {n: int(scalars[k]) for k, n in enumerate(qc.SCALARS)} == T.HAND_SCALARS
        assert got.text(qc.TEXT_FLAGSTAT) == T.HAND_FLAGSTAT and got.text(qc.TEXT_STATS) == T.HAND_STATS
        got.reset()
    bt = capi.Batch(toy[1], 1000, 1000 * 160)                                   # the same records from a batch, in HBM
    try:
        assert bt.bam_upload(data) == len(T.HAND)
        for lanes, got in ((True, a), (False, b)):
            way(lanes)
            assert got.add_batch(bt) == 9
            same(got, want)
            assert got.text(qc.TEXT_STATS) == T.HAND_STATS
    finally:
        bt.close()
    empty = capi.Batch(toy[1], 10, 1000)
    assert capi.lib().bwams_qc_add_batch(a.h, empty.h, None) == ERR_ARG         # neither bam_run nor bam_upload
    empty.close()
    for got in (a, b):
        got.close()


def test_cycle_block_edges(way):
    rng = np.random.default_rng(3)
    mc = 128
    recs = []
    for n in (0, 1, 2, 63, 64, 65, mc - 1, mc, mc + 1):
        for flag in (0, 0x10, 0x80, 0x90):                                      # both strands, both classes
            q = [int(v) for v in rng.choice([0, 62, 63, 64, 254, 7, 30, 41], n)]
            recs.append(qrec(flag, 0, 5, 60, -1, -1, 0, [(n, 0)] if n else "", rng.integers(0, 16, n), q))
    for k, n in enumerate((1, 63, 65, mc + 1)):                                 # without qualities, among records with them
        recs.insert(7 * k + 2, qrec(0x10 * (k & 1) | 0x80 * (k >> 1), 0, 5, 60, -1, -1, 0, [(n, 0)], rng.integers(0, 16, n), None))
    recs.append(qrec(0x10, 0, 5, 60, -1, -1, 0, "5M", [1, 2, 4, 8, 15], [0, 62, 63, 64, 254]))
    want, a, b = both(way, [b"".join(recs)], max_cycle=mc, max_isize=10)
    s = {n: int(want.scalars[k]) for k, n in enumerate(qc.SCALARS)}
    assert s["no_qual"] == 4 and s["bases_over"] == 4 + 1 and a.info()["bases_over"] == 5
    qual = want.table(qc.QUAL).reshape(2, mc, 64)
    assert qual[0, 0, 63] >= 1 and qual[0, 4, 0] >= 1 and qual[:, mc - 1].sum() == 8 and qual[:, :, 63].sum() > 20
    assert want.table(qc.BASE).reshape(2, mc, 5)[0, :5].sum(0).tolist() != [0] * 5
    for got in (a, b):
        got.close()


def test_table_edges(way):
    rng = np.random.default_rng(5)
    probe = capi.Qc()
    w = probe.info()["isize_lds"]
    probe.close()
    mi = 3 * w                                                                   # max_isize past the LDS window
    recs = []
    for tlen in (w - 1, w, w + 1, mi - 1, mi, mi + 1, 0, -7, 1):
        for flag, pos, npos in ((0x21, 10, 90), (0x11, 10, 90), (0x21, 90, 10), (0x11, 90, 10), (0x31, 10, 90), (0x01, 10, 90)):
            recs.append(qrec(flag | 0x40, 0, pos, 60, 0, npos, tlen, "2M", "AC", [30, 30]))
    recs.append(qrec(0x21, 0, 10, 60, 1, 90, 50, "2M", "AC", [30, 30]))          # another reference: no insert size
    recs.append(qrec(0x21, -1, 10, 60, -1, 90, 50, "2M", "AC", [30, 30]))        # refID -1
    recs.append(qrec(0x29, 0, 10, 60, 0, 90, 50, "2M", "AC", [30, 30]))          # the mate unmapped
    for mapq in (0, 255, 255, 1):
        recs.append(qrec(0, 0, 5, mapq, -1, -1, 0, "1M", "A", [30]))
    for n in (1, 63, 64, 65, 300):
        for op in (1, 2):
            ops = [(2, 0), (n, op), (2, 0)]
            l_seq = 4 + (n if op == 1 else 0)
            recs.append(qrec(0, 0, 5, 60, -1, -1, 0, ops, rng.integers(0, 16, l_seq), [30] * l_seq))
    recs.append(qrec(0, 0, 5, 60, -1, -1, 0, [(0, 1), (0, 2), (1, 0)], "A", [30]))      # I and D of length 0 count nowhere
    ops = [(3, 4)] + [(int(rng.integers(1, 4)), op) for _ in range(40) for op in (0, 1, 0, 2)] + [(2, 4), (5, 5)]     # 163 ops
    l_seq = sum(n for n, op in ops if op in (0, 1, 4))
    recs.append(qrec(0, 0, 5, 60, -1, -1, 0, ops, rng.integers(0, 16, l_seq), [int(v) for v in rng.integers(0, 94, l_seq)], nm=40))
    want, a, b = both(way, [b"".join(recs)], max_isize=mi)
    isize = want.table(qc.ISIZE).reshape(3, mi + 1)
    assert isize[:, [w - 1, w, w + 1, mi - 1]].tolist() == [[2] * 4, [2] * 4, [2] * 4] and isize[:, mi].tolist() == [4, 4, 4]
    assert isize.sum() == 6 * 7 and want.table(qc.MAPQ)[[0, 1, 255]].tolist() == [1, 1, 2]
    indel = want.table(qc.INDEL).reshape(2, 65)
    assert indel[:, 63].tolist() == [1, 1] and indel[:, 1].min() > 1
    assert indel[:, 64].tolist() == [3, 3] and indel[:, 0].tolist() == [0, 0] and want.scalars[4] == 5
    for got in (a, b):
        got.close()
    small = [qrec(0x61, 0, 10, 60, 0, 90, t, "2M", "AC", [30, 30]) for t in (1, 49, 50, 51, 2000)]      # max_isize inside the window
    want, a, b = both(way, [b"".join(small)], max_isize=50)
    assert want.table(qc.ISIZE).reshape(3, 51)[0, [1, 49, 50]].tolist() == [1, 1, 3]
    for got in (a, b):
        got.close()


def _random_record(rng):
    """every FLAG bit, every op, clamped and unclamped values; SEQ and CIGAR need not agree (no rule asks for it)"""
    flag = int(rng.integers(0, 4096))
    ops = [(int(rng.integers(0, 80)), int(rng.choice([0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8]))) for _ in range(int(rng.integers(0, 8)))]
    l_seq = int(rng.choice([0, 1, 30, 64, 100, 151, 200, 530]))
    qual = None if rng.random() < 0.1 else [int(q) for q in rng.integers(0, 100, l_seq)]
    aux = b""
    if rng.random() < 0.7:
        t = [b"c", b"C", b"s", b"S", b"i", b"I"][int(rng.integers(0, 6))]
        aux = (T.B_ARRAY if rng.random() < 0.3 else b"") + aux_int(b"NM", t, int(rng.integers(-3 if t in b"csi" else 0, 100))) + b"XZZab\0"
    refid, nref = int(rng.integers(-1, 2)), int(rng.integers(-1, 2))
    return qrec(flag, refid, int(rng.integers(0, 5000)), int(rng.choice([0, 4, 5, 60, 255])), nref, int(rng.integers(0, 5000)),
                int(rng.integers(-50, 9000)), ops, rng.integers(0, 16, l_seq), qual, aux=aux)


def test_record_counts(way):
    rng = np.random.default_rng(9)
    probe = capi.Qc()
    slice_ = probe.info()["slice"]
    probe.close()
    one = qrec(0x10, 0, 5, 60, -1, -1, 0, "70M", rng.integers(0, 16, 70), [int(q) for q in rng.integers(0, 70, 70)], nm=1)
    for adds in ([b""], [one], [b"", one, b""]):
        want, a, b = both(way, adds, max_cycle=64)
        assert want.flags[0, 0] == sum(1 for d in adds if d)
        for got in (a, b):
            got.close()
    recs = [qrec(0x80 * (k % 3 == 0) | 0x10 * (k % 5 == 0), 0, 5, 60, -1, -1, 0, "3M", [1 << (k % 4)] * (1 + k % 70), [k % 50] * (1 + k % 70))
            for k in range(next(n for n in range(4 * slice_) if n - (n + 2) // 3 == slice_ + 1))]      # class 0 holds one more than a slice
    assert sum(1 for k in range(len(recs)) if k % 3) == slice_ + 1
    want, a, b = both(way, [b"".join(recs)])
    for got in (a, b):
        got.close()
    pile = qrec(0x63, 0, 10, 60, 0, 90, 300, "2S60M2I60M1D27M", rng.integers(0, 16, 151), [30] * 151, nm=2) * 5000      # contention
    want, a, b = both(way, [pile, pile])
    assert want.table(qc.QUAL).reshape(2, 512, 64)[0, 150, 30] == 10000 and want.table(qc.ISIZE).reshape(3, 8001)[0, 300] == 10000
    for got in (a, b):
        got.close()
    data = b"".join(_random_record(rng) for _ in range(4000))
    want, a, b = both(way, [data])
    assert (want.flags[:, 1:] > 5).all() and want.scalars[9] > 0 and want.scalars[6] > 100 and want.scalars[5] > 1000
    assert want.table(qc.ISIZE).sum() > 5 and (want.table(qc.INDEL).reshape(2, 65)[:, 64] > 0).all()
    for got in (a, b):
        got.close()


@pytest.mark.parametrize("tag,data,at,why", T.refusals(), ids=[r[0] for r in T.refusals()])
def test_refusals(way, tag, data, at, why):
    L = capi.lib()
    before = T.GOOD * 3
    want = qc.Qc()
    want.add(before)
    text = {"l_seq": "has a negative l_seq or a CIGAR that ends behind the record (bounds)", "op": "has a CIGAR op code above 8 (op)",
            "both": "has a CIGAR op code above 8 (op)", "qual": "ends inside its SEQ or QUAL (bounds)"}.get(
                tag, "has an aux area that cannot be walked (aux)")
    for lanes in (True, False):
        way(lanes)
        got = capi.Qc()
        assert got.add_records(before) == 3
        n = C.c_int64(-1)
        assert L.bwams_qc_add_records(got.h, data, len(data), C.byref(n)) == ERR_ARG
        if tag == "cigar":                                                       # the block_size chain's check sees this one first
            assert L.bwams_last_error().decode().startswith("bwams_qc_add_records: record %d" % at)
        else:
            assert L.bwams_last_error().decode() == "bwams_qc_add_records: record %d %s" % (at, text)
        same(got, want)                                                          # nothing of the call was added
        got.close()


def test_state_and_arguments(way):
    L = capi.lib()
    rng = np.random.default_rng(12)
    recs = [_random_record(rng) for _ in range(600)]
    whole = qc.Qc()
    whole.add(b"".join(recs))
    want, a, b = both(way, [b"".join(recs[:100]), b"", b"".join(recs[100:101]), b"".join(recs[101:])])
    for got in (a, b):
        same(got, whole)                                                         # several adds are one add
        got.reset()
        same(got, qc.Qc())
        assert got.text(qc.TEXT_FLAGSTAT) == T.EMPTY_FLAGSTAT and got.text(qc.TEXT_STATS) == T.EMPTY_STATS
        assert got.add_records(b"".join(recs)) == want.scalars[0]
        same(got, whole)
    n = C.c_int64(0)
    buf = np.zeros(70000, np.int64)
    vp = buf.ctypes.data_as(C.c_void_p)
    sizes = [2 * 513, 2 * 512 * 64, 2 * 512 * 5, 256, 3 * 8001, 130]
    for what, size in enumerate(sizes):
        assert L.bwams_qc_table(a.h, what, None, 0, C.byref(n)) == 0 and n.value == size          # NULL: the size
        assert L.bwams_qc_table(a.h, what, vp, size - 1, C.byref(n)) == ERR_CAPACITY and n.value == size
        assert L.bwams_qc_table(a.h, what, vp, size, None) == 0 and np.array_equal(buf[:size], whole.table(what))
    assert L.bwams_qc_table(a.h, 6, vp, 70000, C.byref(n)) == ERR_ARG and L.bwams_qc_table(a.h, -1, vp, 70000, C.byref(n)) == ERR_ARG
    assert L.bwams_qc_table(a.h, 0, vp, -1, C.byref(n)) == ERR_ARG and L.bwams_qc_table(None, 0, vp, 70000, C.byref(n)) == ERR_ARG
    text = whole.text(qc.TEXT_FLAGSTAT)
    out = C.create_string_buffer(4096)
    assert L.bwams_qc_text(a.h, 0, None, 0, C.byref(n)) == ERR_CAPACITY and n.value == len(text)
    assert L.bwams_qc_text(a.h, 0, out, len(text) - 1, C.byref(n)) == ERR_CAPACITY and n.value == len(text)
    assert L.bwams_qc_text(a.h, 0, out, len(text), C.byref(n)) == 0 and out.raw[:n.value].decode() == text
    assert L.bwams_qc_text(a.h, 2, out, 4096, C.byref(n)) == ERR_ARG and L.bwams_qc_text(None, 0, out, 4096, C.byref(n)) == ERR_ARG
    assert L.bwams_qc_summary(a.h, None) == ERR_ARG and L.bwams_qc_info(a.h, None) == ERR_ARG and L.bwams_qc_reset(None) == ERR_ARG
    cut = T.GOOD[:-1]
    assert L.bwams_qc_add_records(a.h, cut, len(cut), None) == ERR_ARG          # the chain, as bwams_bam_upload checks it
    assert L.bwams_qc_add_records(a.h, None, 5, None) == ERR_ARG
    for got in (a, b):
        got.close()
    h = C.c_void_p()
    for o in (capi.QcOpt(0x10000, 512, 8000, 0), capi.QcOpt(0x900, 0, 8000, 0), capi.QcOpt(0x900, 100, 8000, 0), capi.QcOpt(0x900, 4160, 8000, 0),
              capi.QcOpt(0x900, 512, 0, 0), capi.QcOpt(0x900, 512, (1 << 20) + 1, 0), capi.QcOpt(0x900, 512, 8000, 1)):
        assert L.bwams_qc_open(0, C.byref(o), C.byref(h)) == ERR_ARG
    assert L.bwams_qc_open(0, None, None) == ERR_ARG
    assert L.bwams_qc_open(0, None, C.byref(h)) == 0                            # NULL: the defaults
    assert L.bwams_qc_table(h, qc.ISIZE, None, 0, C.byref(n)) == 0 and n.value == 3 * 8001
    assert L.bwams_qc_close(h) == 0 and L.bwams_qc_close(None) == 0
    big = capi.Qc(exclude=0, max_cycle=4096, max_isize=1 << 20)                 # the largest tables, and no filter
    long = qrec(0x900 | 0x10, 0, 5, 60, -1, -1, 0, "4100M", rng.integers(0, 16, 4100), [int(q) for q in rng.integers(0, 94, 4100)])
    far = qrec(0x61, 0, 10, 60, 0, 90, (1 << 20) + 5, "2M", "AC", [1, 2])
    w = qc.Qc(exclude=0, max_cycle=4096, max_isize=1 << 20)
    for lanes in (True, False):
        way(lanes)
        assert big.add_records(long + far) == w.add(long + far) == 2
        same(big, w)
    assert w.scalars[9] == 8 and w.table(qc.ISIZE).reshape(3, -1)[0, 1 << 20] == 2
    big.close()


def test_from_a_real_batch(way, toy):
    from test_gpu_markdup import _pe_chunk
    g, ix = toy
    t1, t2, _ = _pe_chunk(g, 1200, 8)
    b = capi.Batch(ix, 4000, 4000 * 160)
    try:
        b.process_chunk2(t1, t2)
        b.bam_run()
        raw, _ = b.bam_fetch()
        want = qc.Qc()
        n = want.add(raw)
        assert n > 2000 and want.flags[0, 11] > 1500 and want.insert_size()[0] > 500 and want.scalars[6] == 0 and want.scalars[2] > 2000
        for lanes in (True, False):
            way(lanes)
            got = capi.Qc()
            assert got.add_batch(b) == n
            same(got, want)
            got.close()
    finally:
        b.close()


def _sorter(tmp_path, tag, ix, hdr, runs, q=None, p=None, d=None, markdup=True):
    path = str(tmp_path / ("%s.bam" % tag))
    s = capi.Sorter(path, 0, hdr, markdup=markdup)
    b = capi.Batch(ix, 1000, 1000 * 160)
    try:
        if q is not None:
            s.set_qc(q)
        if p is not None:
            s.set_pileup(p)
        if d is not None:
            s.set_depth(d)
        for k, run in enumerate(runs):
            b.bam_upload(run)
            s.put_batch(k, b)
            if k == 0 and q is not None:
                assert capi.lib().bwams_sorter_set_qc(s.h, q.h) == ERR_ARG      # after a put
                assert capi.lib().bwams_last_error().decode() == "bwams_sorter_set_qc: called after the sorter's first put"
    finally:
        st = s.close()
        b.close()
    return open(path, "rb").read(), open(path + ".bai", "rb").read(), st


def _fragment(k: int, refid: int, pos: int, flag: int = 0, qual: int = 40, pad: int = 0) -> bytes:
    return rec(refid, pos, "100M", flag=flag, name=b"f%d" % k, qual=qual, pad=pad)          # SEQ: 100 A


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
    q1, q3 = capi.Qc(exclude=0xD00), capi.Qc(exclude=0xD00)                     # duplicates filtered out of the tables
    p3, d3 = capi.Pileup(l_ref), capi.Depth(l_ref)
    data0, x0, st0 = _sorter(tmp_path, "plain", ix, hdr, runs)
    data1, x1, st1 = _sorter(tmp_path, "qc", ix, hdr, runs, q=q1)
    data3, x3, _ = _sorter(tmp_path, "all", ix, hdr, runs, q=q3, p=p3, d=d3)
    data2, x2, _ = _sorter(tmp_path, "two", ix, hdr, runs, p=p3, d=None)
    assert data0 == data1 == data2 == data3 and x0 == x1 == x2 == x3            # the file and its index do not know about the handles
    written = gzip.decompress(data0)[len(hdr):]
    want = qc.Qc(exclude=0xD00)
    n = want.add(written)
    assert st1.dup.records_marked >= 1 and n == st1.records - st1.dup.records_marked
    assert want.flags[0, 4] == st1.dup.records_marked and want.flags[0, 0] == st1.records == 2403
    for q in (q1, q3):
        same(q, want)
    asgiven = qc.Qc(exclude=0xD00)
    asgiven.add(b"".join(runs))
    assert asgiven.flags[0, 4] == 1 and asgiven.scalars[0] == 2402              # the stale mark; the real duplicate was not marked yet
    assert np.array_equal(d3.finish().fetch(1), p3.fetch(1)[:, :8].sum(1) // 2)              # p3 saw the stream twice, d3 once
    L = capi.lib()
    s = capi.Sorter(str(tmp_path / "args.bam"), 0, hdr)
    assert L.bwams_sorter_set_qc(s.h, None) == ERR_ARG and L.bwams_sorter_set_qc(None, q1.h) == ERR_ARG
    n_dev = C.c_int(0)
    L.bwams_device_count(C.byref(n_dev))
    if n_dev.value > 1:                                                         # with one GPU this case does not run
        far = capi.Qc(device=1)
        assert L.bwams_sorter_set_qc(s.h, far.h) == ERR_ARG                     # another device
        far.close()
    assert L.bwams_sorter_set_qc(s.h, q1.h) == 0                                # no lengths to compare: any handle of the device
    s.close()
    for h in (q1, q3, p3, d3):
        h.close()


def test_sorter_record_across_pieces(tmp_path, toy):
    """just over one deflate piece of records: one straddles the cut and is counted once, with the flag the merge gave it.  Every
    record is 100M of A with quality 30 on the forward strand, so every counter has a closed form."""
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
    q = capi.Qc(exclude=0xD00)
    data, _, st = _sorter(tmp_path, "cut", ix, hdr, runs, q=q)
    assert st.records == n and st.dup.records_marked == 0
    flags, s = q.summary()
    assert flags[0].tolist() == [n, n, 0, 0, 0, 0, n, n] + [0] * 8 and not flags[1].any()
    assert s[:11].tolist() == [n, 100 * n, n, 100 * n, 0, 0, n, 3000 * n, 100 * n, 0, 0]
    base, qual = q.table(qc.BASE).reshape(2, 512, 5), q.table(qc.QUAL).reshape(2, 512, 64)
    assert (base[0, :100, 0] == n).all() and base.sum() == 100 * n and (qual[0, :100, 30] == n).all() and qual.sum() == 100 * n
    assert q.table(qc.RL)[100] == n and q.table(qc.MAPQ)[60] == n
    q.close()
