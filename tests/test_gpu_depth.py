"""Depth of coverage on the GPU (csrc/depth.hip, csrc/api_depth.hip, host/bam_sort.cpp's bwams_sorter_set_depth) through the C-ABI,
compared exactly with bwams/depth.py's restatement of the rules and with the hand-written expectations of tests/test_depth.py."""
import ctypes as C
import gzip
import struct

import numpy as np
import pytest

from bwams import bam, capi, depth, simulate
import test_depth as T
from test_depth import rec

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


@pytest.fixture(scope="module")
def batch(toy):
    b = capi.Batch(toy[1], 1000, 1000 * 160)
    yield b
    b.close()


def same(got: capi.Depth, want: depth.Depth, bins=(2, 7, 300), ws=(1, 3, 64, 1000)):
    """every query of a finished handle against the restatement"""
    n_ref = len(want.l_ref)
    for r in range(n_ref):
        assert np.array_equal(got.fetch(r), want.depth[r]), r
    rows = got.summary()
    assert [{k: int(x[k]) for k in ("length", "bases", "min", "max")} for x in rows] == want.summary()
    for nb in bins:
        for r in [-1] + list(range(min(n_ref, 4))) + ([n_ref - 1] if n_ref > 4 else []):
            assert np.array_equal(got.hist(r, nb), want.hist(r, nb)), (r, nb)
    for w in ws:
        assert np.array_equal(got.windows(w), want.windows(w)), w
    for r in list(range(min(n_ref, 4))) + ([n_ref - 1] if n_ref > 4 else []):
        s, v = got.runs(r, 0, want.l_ref[r])
        ws_, wv = want.runs(r, 0, want.l_ref[r])
        assert np.array_equal(s, ws_) and np.array_equal(v, wv), r


def both(l_ref, data: bytes, **kw):
    """a finished device handle and restatement of one add of `data`"""
    want = depth.Depth(l_ref, **kw)
    n = want.add(data)
    got = capi.Depth(l_ref, **kw)
    assert got.add_records(data) == n
    return got.finish(), want.finish()


def test_hand_records(batch):
    data = b"".join(T.HAND)
    for dels, lit in ((False, T.WANT), (True, T.WANT_DEL)):
        got, want = both(T.L_REF, data, count_deletions=dels)
        assert [got.fetch(r).tolist() for r in range(4)] == lit
        same(got, want, ws=(1, 8, 12, 20, 100))
        got.close()
    got = capi.Depth(T.L_REF)                                                   # the same records from a batch, in HBM
    assert batch.bam_upload(data) == len(T.HAND)
    assert got.add_batch(batch) == T.N_COUNTED
    got.finish()
    assert [got.fetch(r).tolist() for r in range(4)] == T.WANT
    assert got.text(T.NAMES, depth.TEXT_SUMMARY) == T.TEXT_SUMMARY
    assert got.text(T.NAMES, depth.TEXT_DIST) == T.TEXT_DIST
    assert got.text(T.NAMES, depth.TEXT_WINDOWS, 8) == T.TEXT_WINDOWS_8
    got.close()
    ex = capi.Depth(T.EX_L_REF)
    ex.add_records(b"".join(T.EX_RECS))
    ex.finish()
    assert ex.text(T.EX_NAMES, 0) == T.EX_SUMMARY and ex.text(T.EX_NAMES, 1) == T.EX_DIST and ex.text(T.EX_NAMES, 2, 4) == T.EX_WINDOWS_4
    n = C.c_int64(0)
    assert capi.lib().bwams_depth_text(ex.h, b"c1\0c2\0", 0, 0, None, 0, C.byref(n)) == ERR_CAPACITY and n.value == len(T.EX_SUMMARY)
    assert capi.lib().bwams_depth_text(ex.h, b"c1\0c2\0", 3, 0, None, 0, C.byref(n)) == ERR_ARG
    ex.close()


def _random_cigar(rng, n_ops):
    """every op; S and H only at the ends, as SAM has them; neighbours that merge (M = X, M I M, M P M) and that must not (M N M, M D M)"""
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


def test_cigar_ops():
    rng = np.random.default_rng(5)
    l_ref = [3001, 2500]
    recs = [rec(int(rng.integers(0, 2)), int(rng.integers(0, 3100)), _random_cigar(rng, int(rng.integers(1, 12)))) for _ in range(3000)]
    recs.append(rec(0, 5, [(1, 0), (0, 3)] * 1500))                             # 3000 ops: M N(0) M ... every stretch apart
    recs.append(rec(1, 100, [(1, int(rng.choice([0, 1, 2, 7, 8]))) for _ in range(3000)]))
    recs.append(rec(0, 700, "3H2S4M2N4M1D1=1X1I1M1P2M2S3H"))
    for dels in (False, True):
        got, want = both(l_ref, b"".join(recs), count_deletions=dels)
        same(got, want)
        got.close()
    a, w = both(l_ref, rec(0, 10, "4M2N4M"))                                    # M N M: the gap stays empty
    assert a.fetch(0, 8, 22).tolist() == [0, 0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 0, 0]
    a.close()


def test_reference_edges():
    rng = np.random.default_rng(11)
    l_ref = [int(x) for x in rng.integers(1, 6, 300)] + [7001]                  # 300 tiny references, then one over several 2048-slot pieces
    l_ref[17], l_ref[18] = 1, 0
    recs = []
    for r in range(300):
        for _ in range(3):
            recs.append(rec(r, int(rng.integers(-1, 7)), [(int(rng.integers(1, 8)), 0)]))
    k = 40
    recs += [rec(k, 0, [(l_ref[k], 0)]),                                        # ends exactly at l_ref
             rec(k, l_ref[k] - 1, "1M"),                                        # starts at l_ref - 1
             rec(k, l_ref[k] - 1, "9M"),                                        # runs past the end: clipped
             rec(k, l_ref[k], "4M"), rec(k, l_ref[k] + 50, "4M"),               # POS at and beyond l_ref
             rec(k + 1, 0, "1M"),                                               # base 0 of the next reference
             rec(17, 0, "3M"), rec(18, 0, "3M"),                                # a reference of one base, and one of none
             rec(300, 7000, "5M"), rec(300, 0, "7001M"), rec(300, 2040, "20M"), rec(300, 4090, "10M"), rec(299, 0, "9M")]
    got, want = both(l_ref, b"".join(recs))
    same(got, want, ws=(1, 2, 5, 7001, 100000))
    lone, w1 = both(l_ref, rec(k, l_ref[k] - 1, "9M") + rec(k + 2, 0, "1M"))    # neither leaks into reference k + 1
    assert lone.fetch(k).tolist() == [0] * (l_ref[k] - 1) + [1] and not lone.fetch(k + 1).any() and lone.fetch(k + 2, 0, 1).tolist() == [1]
    same(lone, w1, bins=(2,), ws=(1,))
    for d in (got, lone):
        d.close()


def test_filters():
    L = capi.lib()
    for bit in (0x4, 0x100, 0x200, 0x400):
        got, want = both([10], rec(0, 0, "3M", flag=bit) + rec(0, 0, "1M", flag=0x1 | 0x10 | 0x800))
        assert got.fetch(0).tolist() == [1] + [0] * 9
        got.close()
    got, want = both([10], rec(0, 0, "3M", flag=0x800) + rec(0, 0, "1M") + rec(0, 2, "2M", flag=0x400), exclude=0x800)
    assert got.fetch(0).tolist() == [1, 0, 1, 1] + [0] * 6
    got.close()
    got, want = both([10], rec(0, 0, "3M", mapq=29) + rec(0, 1, "3M", mapq=30), min_mapq=30)
    assert got.fetch(0).tolist() == [0, 1, 1, 1] + [0] * 6
    got.close()
    d = capi.Depth([10, 10])
    assert d.add_records(rec(-1, 0, "3M") + rec(2, 0, "3M") + rec(0, 0, "") + rec(1, 4, "2M")) == 1      # skipped, not refused
    n = C.c_int64(7)
    bad = rec(0, 0, "5M") + rec(1, 0, "5M") * 70 + rec(1, 0, [(2, 0), (1, 9)]) + rec(0, 0, [(1, 15)])
    assert L.bwams_depth_add_records(d.h, bad, len(bad), C.byref(n)) == ERR_ARG
    assert L.bwams_last_error().decode() == "bwams_depth_add_records: record 71 has a CIGAR op code above 8"
    d.finish()
    assert d.fetch(0).tolist() == [0] * 10 and d.fetch(1).tolist() == [0, 0, 0, 0, 1, 1, 0, 0, 0, 0]     # what it was before the refusal
    d.close()
    cut = rec(0, 0, "5M")[:-1]
    d = capi.Depth([10])
    assert L.bwams_depth_add_records(d.h, cut, len(cut), None) == ERR_ARG       # the chain, as bwams_bam_upload checks it
    d.close()


def test_contention():
    n = 70001                                                                   # no multiple of 64
    rng = np.random.default_rng(3)
    l_ref = [9000, 4000]
    spread = [rec(int(p) % 2, int(p), "100M") for p in rng.integers(0, 8950, n)]
    data = rec(1, 1234, "75M2D25M") * n + b"".join(spread)
    got, want = both(l_ref, data)
    assert int(got.summary()["max"][1]) > 65535
    same(got, want, bins=(2, 65536, 70001, 75000), ws=(1, 1000))
    assert got.hist(1, 65536)[65535] == want.hist(1, 65536)[65535] >= 100
    sorted_ = depth.Depth(l_ref)                                                # coordinate order: neighbours in a wave share slots
    recs = sorted(spread, key=lambda r: struct.unpack_from("<ii", r, 4))
    sorted_.add(b"".join(recs))
    g2 = capi.Depth(l_ref)
    g2.add_records(b"".join(recs))
    same(g2.finish(), sorted_.finish(), bins=(300,), ws=(64,))
    empty, w0 = both(l_ref, b"")
    assert not empty.fetch(0).any() and empty.hist(-1, 2).tolist() == [13000, 0]
    same(empty, w0)
    none = capi.Depth([]).finish()                                              # no reference at all
    assert len(none.summary()) == 0 and none.windows(5).tolist() == [] and none.hist(-1, 2).tolist() == [0, 0]
    for d in (got, g2, empty, none):
        d.close()


def test_without_the_fold(monkeypatch):
    """BWAMS_DEPTH_COMBINE=0 (one atomic per lane, tools/depth_rate.py's 'without' column) gives the same depths"""
    rng = np.random.default_rng(13)
    l_ref = [3001, 2500]
    recs = [rec(int(rng.integers(0, 2)), int(rng.integers(0, 3100)), _random_cigar(rng, int(rng.integers(1, 12)))) for _ in range(2000)]
    data = rec(1, 77, "60M3D40M") * 1001 + b"".join(recs)
    monkeypatch.setenv("BWAMS_DEPTH_COMBINE", "0")
    capi.debug_reload()
    for dels in (False, True):
        got, want = both(l_ref, data, count_deletions=dels)
        same(got, want, bins=(2, 2000))
        got.close()


def test_accumulation_and_state(batch):
    L = capi.lib()
    data = b"".join(T.HAND)
    d = capi.Depth(T.L_REF)
    buf = np.zeros(64, np.int64)
    assert L.bwams_depth_summary(d.h, buf.ctypes.data_as(C.c_void_p), 4) == ERR_ARG          # a query before finish
    assert L.bwams_depth_hist(d.h, -1, buf.ctypes.data_as(C.c_void_p), 4) == ERR_ARG
    assert L.bwams_depth_fetch(d.h, 0, 0, 1, buf.ctypes.data_as(C.c_void_p)) == ERR_ARG
    parts = (T.HAND[:5], T.HAND[5:11], T.HAND[11:])
    assert sum(d.add_records(b"".join(p)) for p in parts) == T.N_COUNTED
    d.finish()
    d.finish()                                                                  # a second finish does nothing
    assert [d.fetch(r).tolist() for r in range(4)] == T.WANT
    assert L.bwams_depth_add_records(d.h, data, len(data), None) == ERR_ARG     # an add after finish
    batch.bam_upload(data)
    assert L.bwams_depth_add_batch(d.h, batch.h, None) == ERR_ARG
    d.reset()
    assert L.bwams_depth_fetch(d.h, 0, 0, 1, buf.ctypes.data_as(C.c_void_p)) == ERR_ARG
    d.add_records(b"".join(T.HAND[:3]))
    d.finish()
    fresh, want = both(T.L_REF, b"".join(T.HAND[:3]))
    assert [d.fetch(r).tolist() for r in range(4)] == [fresh.fetch(r).tolist() for r in range(4)]
    same(d, want, ws=(1, 8))
    for x in (d, fresh):
        x.close()


def test_queries():
    lds = 4096                                                                  # csrc/common.h: kDepthHistLds
    rng = np.random.default_rng(9)
    l_ref = [30011, 4099]                                                       # the scan's carries cross several blocks
    # reference 1: depths lds - 2 .. lds + 1 side by side (each block of 10 bases one deeper), over a floor of random reads on reference 0
    data = rec(1, 100, "40M") * (lds - 2) + rec(1, 110, "30M") + rec(1, 120, "20M") + rec(1, 130, "10M")
    data += b"".join(rec(0, int(p), "150M") for p in rng.integers(0, 29900, 3000))
    got, want = both(l_ref, data)
    assert got.fetch(1, 100, 140)[::10].tolist() == [lds - 2, lds - 1, lds, lds + 1]
    same(got, want, bins=(2, lds - 1, lds, lds + 1, lds + 2, lds + 3, 5000), ws=(1, 4099, 4100, 30011, 1000, 7))
    s, v = got.runs(1, 105, 135)                                                # starts inside the first run
    assert s.tolist() == [105, 110, 120, 130] and v.tolist() == [lds - 2, lds - 1, lds, lds + 1]
    ws_, wv = want.runs(0, 777, 20000)
    s, v = got.runs(0, 777, 20000)
    assert np.array_equal(s, ws_) and np.array_equal(v, wv) and s[0] == 777
    with pytest.raises(capi.BwamsError) as e:
        got.runs(0, 777, 20000, cap=len(ws_) - 1)
    assert e.value.code == ERR_CAPACITY and got.n_runs == len(ws_)
    s, v = got.runs(0, 777, 20000, cap=len(ws_))
    assert np.array_equal(s, ws_)
    assert got.runs(0, 5, 5)[0].tolist() == []
    L = capi.lib()
    buf = np.zeros(8, np.int64)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.bwams_depth_hist(got.h, 2, p, 4) == ERR_ARG and L.bwams_depth_hist(got.h, 0, p, 1) == ERR_ARG
    assert L.bwams_depth_windows(got.h, 0, p, 8, None) == ERR_ARG and L.bwams_depth_windows(got.h, 5000, p, 1, None) == ERR_CAPACITY
    assert L.bwams_depth_fetch(got.h, 1, 0, 4100, p) == ERR_ARG
    got.close()


def test_from_a_real_batch(toy):
    from test_gpu_markdup import _pe_chunk
    g, ix = toy
    l_ref = [150000, len(g) - 150000]
    t1, t2, planted = _pe_chunk(g, 1200, 8)
    b = capi.Batch(ix, 4000, 4000 * 160)
    try:
        b.process_chunk2(t1, t2)
        b.bam_run()
        before = capi.Depth(l_ref)
        n0 = before.add_batch(b)
        raw, _ = b.bam_fetch()
        w0 = depth.Depth(l_ref)
        assert w0.add(raw) == n0
        st = b.bam_markdup()
        marked, _ = b.bam_fetch()
        after = capi.Depth(l_ref)
        n1 = after.add_batch(b)
        w1 = depth.Depth(l_ref)
        assert w1.add(marked) == n1
        assert st.records_marked > len(planted) // 2 and n1 <= n0 - len(planted) // 2      # the planted duplicates drop out by rule 2
        same(before.finish(), w0.finish(), bins=(2, 40), ws=(1000,))
        same(after.finish(), w1.finish(), bins=(2, 40), ws=(1000,))
        assert int(after.summary()["bases"].sum()) < int(before.summary()["bases"].sum())
        before.close(); after.close()
    finally:
        b.close()


def _fragment(k: int, refid: int, pos: int, flag: int = 0, qual: int = 40, pad: int = 0) -> bytes:
    return rec(refid, pos, "100M", flag=flag, name=b"f%d" % k, qual=qual, pad=pad)


def _sorter(tmp_path, tag, ix, hdr, runs, d, markdup=True):
    path = str(tmp_path / ("%s.bam" % tag))
    s = capi.Sorter(path, 0, hdr, markdup=markdup)
    b = capi.Batch(ix, 1000, 1000 * 160)
    try:
        if d is not None:
            s.set_depth(d)
        for k, run in enumerate(runs):
            b.bam_upload(run)
            s.put_batch(k, b)
            if k == 0 and d is not None:
                assert capi.lib().bwams_sorter_set_depth(s.h, d.h) == ERR_ARG  # after a put
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
    d = capi.Depth(l_ref)
    data, x, st = _sorter(tmp_path, "depth", ix, hdr, runs, d)
    data0, x0, st0 = _sorter(tmp_path, "plain", ix, hdr, runs, None)
    assert data == data0 and x == x0                                            # the file and its index do not know about the handle
    written = gzip.decompress(data)[len(hdr):]
    want = depth.Depth(l_ref)
    n = want.add(written)
    assert st.dup.records_marked >= 1 and n == st.records - st.dup.records_marked
    asgiven = depth.Depth(l_ref)
    asgiven.add(b"".join(runs))
    d.finish()
    same(d, want.finish(), bins=(2, 50), ws=(1, 100))
    assert d.fetch(0, 4000, 4001).tolist() == [1] and d.fetch(1, 2995, 2996).tolist() == [1]         # one of the two; the stale mark gone
    assert asgiven.finish().depth[0][4000] == 2 and asgiven.depth[1][2995] == 0
    d.close()
    L = capi.lib()
    s = capi.Sorter(str(tmp_path / "args.bam"), 0, hdr)
    other = capi.Depth([5000, 3001])
    assert L.bwams_sorter_set_depth(s.h, other.h) == ERR_ARG                    # lengths that are not the header's
    assert L.bwams_last_error().decode() == "bwams_sorter_set_depth: the depth handle's reference lengths are not the sorter header's"
    assert L.bwams_sorter_set_depth(s.h, None) == ERR_ARG
    if _device_count() > 1:                                                     # with one GPU this case, and bwams_depth_add_batch's device check, do not run
        far = capi.Depth(l_ref, device=1)
        assert L.bwams_sorter_set_depth(s.h, far.h) == ERR_ARG                  # another device
        far.close()
    s.close()
    other.close()


def _device_count() -> int:
    n = C.c_int(0)
    capi.lib().bwams_device_count(C.byref(n))
    return n.value


def test_sorter_record_across_pieces(tmp_path, toy):
    """just over two deflate pieces of records: one straddles each cut and is counted once, with the flag the merge gave it"""
    _, ix = toy
    rng = np.random.default_rng(33)
    l_ref = [200000]
    hdr = bam.header_block(b"@HD\tVN:1.6\tSO:coordinate\n", [b"big"], l_ref)
    n = 116000
    pos = np.sort(rng.choice(199000, n, replace=False))                         # distinct places: no duplicates, every stale mark cleared
    recs = [_fragment(k, 0, int(p), flag=0x400 if k % 3 == 0 else 0, qual=30, pad=int(rng.integers(80, 120))) for k, p in enumerate(pos)]
    size = np.cumsum([0] + [len(r) for r in recs])
    assert size[-1] > 2 * PIECE and all(((size[:-1] < c) & (size[1:] > c)).any() for c in (PIECE, 2 * PIECE))   # a straddler at each cut
    runs = [b"".join(recs[k::3]) for k in range(3)]                             # the merge interleaves them back into `recs`
    d = capi.Depth(l_ref)
    data, _, st = _sorter(tmp_path, "cut", ix, hdr, runs, d)
    written = gzip.decompress(data)[len(hdr):]
    assert len(written) == size[-1] and st.dup.records_marked == 0
    want = depth.Depth(l_ref)
    assert want.add(written) == n
    d.finish()
    assert np.array_equal(d.fetch(0), want.finish().depth[0])
    assert int(d.summary()["bases"][0]) == 100 * n
    d.close()
