"""The quality model and its application on the GPU (host/recal_model.cpp, csrc/recal_apply.hip, csrc/api_recal_apply.hip) through the
C-ABI, compared exactly with bwams/recal_apply.py's restatement.  Every comparison covers the whole output bytes, so what lies
outside QUAL too, and the number of records rewritten."""
import ctypes as C

import numpy as np
import pytest

from bwams import bam, capi, recal, simulate
from bwams import recal_apply as A
import test_recal as T
import test_recal_model as M
from test_gpu_recal import random_record, random_ref
from test_recal import rrec

pytestmark = pytest.mark.gpu

ERR_ARG = -3
USED_Q = (6, 7, 20, 30, 37, 41, 93)
TEXT = {"bounds": "ends inside its SEQ or QUAL (bounds)", "cycle": "is longer than the model's max_cycle (cycle)",
        "aux": "has aux fields that do not chain to its end (aux)"}


def header(ids) -> bytes:
    return b"@HD\tVN:1.6\n" + b"".join(b"@RG\tID:%s\n" % i for i in ids)


def random_tables(rng, n_rg: int, max_cycle: int):
    """count tables with cells in the rows of USED_Q only (a model of them costs the restatement little): about half of the CYCLE
    and CONTEXT cells hold counts, with error rates from none to one in three"""
    t = M.zero_tables(n_rg, max_cycle)
    for g in range(n_rg + 1):
        for q in USED_Q:
            for what, n in ((recal.CYCLE, 2 * max_cycle + 1), (recal.CONTEXT, 16)):
                obs = rng.integers(1, 5000, n) * (rng.random(n) < 0.5)
                t[what][g, q, :, 0] = obs
                t[what][g, q, :, 1] = (obs * rng.choice([0, 0.0003, 0.01, 0.3], n)).astype(np.int64)
            t[recal.QUAL][g, q] = t[recal.CYCLE][g, q].sum(0)
        t[recal.RG][g] = t[recal.QUAL][g].sum(0)
    return t


def read(rng, n: int, flag: int = 0, rg=None, odd: float = 0.05, quals=(0, 5, 6, 7, 20, 30, 37, 41, 93, 94, 200, 255), aux=b"NMC\1"):
    """a record of n bases: codes 1 2 4 8 with a share `odd` of 0 and 15, QUAL bytes from `quals` (the first never 0xFF)"""
    seq = [int(c) for c in rng.choice([1, 2, 4, 8], n)]
    for i in np.flatnonzero(rng.random(n) < odd):
        seq[i] = int(rng.choice([0, 15]))
    q = [int(v) for v in rng.choice(quals, n)]
    if q[0] == 255:
        q[0] = 94
    return rrec(0, 7, [(n, 0)], seq, q, flag=flag, rg=rg, aux=aux, name=b"q%d" % n)


def both(tables, max_cycle, ids, data, **opt):
    """the restatement's bytes and count, and the same from a device handle -> (bytes, records rewritten)"""
    model = A.Model(tables, max_cycle, **opt)
    want, n = A.apply(data, model, ids)
    s, p = capi.recal_model_constants()
    assert s.tolist() == A.S[1:] and p.tolist() == A.P
    m = capi.RecalModel(tables, max_cycle, **opt)
    for what in range(4):
        g, w = m.table(what), model.table(what)
        assert g.dtype == np.int16 and g.shape == w.shape and np.array_equal(g, w), what
    groups = capi.DupGroups(header(ids)) if ids is not None else None
    ap = capi.RecalApply(m, groups)
    m.close()                                                                            # the handle holds its own copy
    got, k = ap.records(data)
    i = ap.info()
    assert i["n_rewritten"] == n and i["n_records"] == len(bam.split_records(data))
    assert i["model_bytes"] == sum(model.table(what).size for what in (1, 2, 3))
    assert k == n and len(got) == len(want)
    assert got == want, np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[:8].tolist()
    ap.close()
    return want, n


def test_worked_example_and_zero_model():
    out, n = both(T.example().tables, 10, [b"a"], b"".join(T.EX_RECS))
    assert n == 2 and M.quals(out) == [[25, 25, 25, 25, 25, 24, 25, 25], [25, 25, 23, 25, 25, 25, 25, 25]]
    q = [0, 5, 6, 7, 59, 60, 61, 93, 94, 200, 255]
    out, n = both(M.zero_tables(0, 16), 16, None, rrec(0, 0, "11M", "ACGTACGTACG", q))
    assert n == 1 and M.quals(out) == [[0, 5, 6, 7, 59, 60, 60, 60, 60, 60, 60]]          # min(b, 93, max_q) from 6 on
    out, _ = both(M.zero_tables(0, 16), 16, None, rrec(0, 0, "3M", "ACG", [0, 50, 255]), max_q=40, preserve_below=0)
    assert M.quals(out) == [[1, 40, 40]]


def test_extreme_model():
    recs = [rrec(0, 0, "2M", "AC", [60, 60], rg="g0"), rrec(0, 0, "3M", "CCC", [50, 50, 50]), rrec(0, 0, "2M", "GG", [50, 50], flag=0x10),
            rrec(0, 0, "2M", "AC", [93, 200], flag=0x81, rg="other")]
    out, n = both(M.extreme_tables(), 3, [b"g0"], b"".join(recs))
    assert n == 4 and M.quals(out) == [[60, 1], [50, 60, 60], [60, 50], [60, 1]]          # + 60, both clamps, - 93


def test_lengths_and_strands():
    rng = np.random.default_rng(41)
    mc = 129
    tables = random_tables(rng, 0, mc)
    recs = []
    for n in (1, 2, 63, 64, 65, 127, 128, 129):                                          # odd lengths: SEQ is nibble-packed
        for flag in (0, 0x10, 0x81, 0x91):                                               # both cycle signs, both context directions
            recs.append(read(rng, n, flag))
            recs.append(read(rng, n, flag, aux=[b"", b"XAAx", b"XBCxXCCy", b"XDsab"][int(rng.integers(0, 4))]))        # QUAL at every alignment
    recs.insert(5, rrec(0, 7, "64M", [1] * 64, [0xFF] + [30] * 63))                       # a first byte 0xFF: stays as it is
    recs.insert(9, rrec(0, 7, "6M", [1, 0, 2, 15, 4, 8], [30, 0xFF, 94, 5, 6, 30], flag=0x10))
    out, n = both(tables, mc, None, b"".join(recs))
    assert n == len(recs) - 1
    changed = sum(x != y for x, y in zip(out, b"".join(recs)))
    assert changed > 2000
    long = read(rng, 130)
    L = capi.lib()
    m = capi.RecalModel(tables, mc)
    ap = capi.RecalApply(m)
    buf = np.frombuffer(recs[0] + long, np.uint8).copy()
    assert L.bwams_recal_apply_records(ap.h, buf.ctypes.data_as(C.c_void_p), len(buf), None) == ERR_ARG
    assert L.bwams_last_error().decode() == "bwams_recal_apply_records: record 1 " + TEXT["cycle"]
    assert buf.tobytes() == recs[0] + long
    ap.close()


def test_read_groups():
    rng = np.random.default_rng(42)
    for ids in (None, [b"solo"], [b"b", b"a", b"ab"]):                                   # none, one and three; IDs not in byte order
        names = [None, b"zz"] + (ids or [b"x"])                                          # no RG, an unknown RG, and every known one
        tables = random_tables(rng, len(ids) if ids else 0, 70)
        recs = [read(rng, int(rng.integers(1, 71)), int(rng.choice([0, 0x10, 0x81, 0x91])), rg=names[k % len(names)]) for k in range(150)]
        both(tables, 70, ids, b"".join(recs))
    L = capi.lib()
    m = capi.RecalModel(M.zero_tables(3, 5), 5)
    h = C.c_void_p()
    for g in (None, capi.DupGroups(header([b"a", b"b"]))):                               # a model of three read groups
        assert L.bwams_recal_apply_open(0, m.h, g.h if g else None, C.byref(h)) == ERR_ARG
    assert L.bwams_last_error().decode() == "bwams_recal_apply_open: the model has 3 read groups, the groups table 2"
    m0 = capi.RecalModel(M.zero_tables(0, 5), 5)
    assert L.bwams_recal_apply_open(0, m0.h, capi.DupGroups(header([b"a"])).h, C.byref(h)) == ERR_ARG
    assert L.bwams_recal_apply_open(0, None, None, C.byref(h)) == ERR_ARG and L.bwams_recal_apply_open(0, m0.h, None, None) == ERR_ARG
    assert L.bwams_recal_apply_close(None) == 0 and L.bwams_recal_model_destroy(None) == 0 and L.bwams_recal_apply_info(None, None) == ERR_ARG


def test_record_counts():
    rng = np.random.default_rng(43)
    ids = [b"x", b"y"]
    tables = random_tables(rng, 2, 40)
    pool = [read(rng, int(rng.integers(1, 41)), int(rng.choice([0, 0x10, 0x81, 0x91, 0x400])), rg=[b"x", b"y", None][k % 3]) for k in range(300)]
    for n in (0, 1, 64, 65, 4097):                                                       # a wave of the record kernel, one more, many blocks
        data = b"".join(pool[int(k)] for k in rng.integers(0, len(pool), n))
        assert both(tables, 40, ids, data)[1] == n
    data = b"".join(pool[int(k)] for k in rng.integers(0, len(pool), 4500))
    assert 3000 < both(tables, 40, ids, data, exclude=0x400)[1] < 4096


def test_random_records_with_their_own_model():
    rng = np.random.default_rng(44)
    l_ref = [900, 333, 2000]
    refs = [random_ref(rng, n, 0.02) for n in l_ref]
    ids = [b"r1", b"r2", b"r3"]
    data = b"".join(random_record(rng, refs, ids) for _ in range(2000))
    want = recal.Recal(l_ref, ids, max_cycle=200)
    for k, codes in enumerate(refs):
        want.set_ref(k, codes)
    want.add(data)
    out, n = both(want.tables, 200, ids, data)
    assert 1500 < n < 2000 and sum(x != y for x, y in zip(out, data)) > 50000
    groups = capi.DupGroups(header(ids))                                                 # the same model from the device's tables
    got = capi.Recal(l_ref, groups, max_cycle=200)
    for k, codes in enumerate(refs):
        got.set_ref(k, codes)
    got.add_records(data)
    m = capi.RecalModel.of(got)
    model = A.Model(want.tables, 200)
    for what in range(4):
        assert np.array_equal(m.table(what), model.table(what)), what
    ap = capi.RecalApply(m, groups)
    assert ap.records(data) == (out, n)
    for h in (ap, m, got):
        h.close()


def test_long_records():
    rng = np.random.default_rng(45)
    tables = random_tables(rng, 0, 600)
    recs = [read(rng, 100), read(rng, 500, 0x91), read(rng, 33, 0x10), read(rng, 600, 0x10), read(rng, 417)]
    assert both(tables, 600, None, b"".join(recs))[1] == 5


@pytest.fixture(scope="module")
def toy():
    g = simulate.make_genome(200000, seed=62, repeat_frac=0.0)
    ix = capi.Index.build(g, 0)
    contigs = np.zeros(1, capi.CONTIG_DTYPE)
    contigs["offset"], contigs["len"] = [0], [len(g)]
    ix.set_contigs(contigs)
    ix.set_contig_names(["chrA"])
    yield g, ix
    ix.close()


@pytest.mark.parametrize("tag,data,at,why,groups", M.refusals(), ids=[r[0] for r in M.refusals()])
def test_refusals(toy, tag, data, at, why, groups):
    """each bad record at the last place of a call: the host bytes and the batch's records stay as they were"""
    L = capi.lib()
    data = M.GOOD * 3 + bam.split_records(data)[at]
    tables = M.zero_tables(1 if groups else 0, 20)
    ids = [b"a"] if groups else None
    with pytest.raises(A.ApplyRefusal) as e:
        A.apply(data, A.Model(tables, 20), ids)
    assert (e.value.record, e.value.why) == (3, why)
    b = capi.Batch(toy[1], 100, 100 * 160)
    try:
        m = capi.RecalModel(tables, 20)
        ap = capi.RecalApply(m, capi.DupGroups(header(ids)) if groups else None)
        buf = np.frombuffer(data, np.uint8).copy()
        n = C.c_int64(-1)
        assert L.bwams_recal_apply_records(ap.h, buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(n)) == ERR_ARG
        assert L.bwams_last_error().decode() == "bwams_recal_apply_records: record 3 " + TEXT[why]
        assert buf.tobytes() == data and n.value == -1
        assert b.bam_upload(data) == 4
        assert L.bwams_recal_apply_batch(ap.h, b.h, C.byref(n)) == ERR_ARG
        assert L.bwams_last_error().decode() == "bwams_recal_apply_batch: record 3 " + TEXT[why]
        assert b.bam_fetch()[0] == data
        ap.close()
    finally:
        b.close()


def test_batch(toy):
    rng = np.random.default_rng(46)
    L = capi.lib()
    tables = random_tables(rng, 1, 60)
    model = A.Model(tables, 60, exclude=0x400)
    recs = [rrec(0, int(rng.integers(0, 5000)), [(n, 0)], [int(c) for c in rng.choice([1, 2, 4, 8, 15], n)],
                 [int(v) for v in rng.choice([3, 6, 20, 30, 41, 93, 200], n)], flag=int(rng.choice([0, 0x10, 0x91, 0x400])),
                 rg=[b"a", None][k % 2], name=b"b%d" % k) for k, n in enumerate(rng.integers(1, 61, 700))]
    data = b"".join(recs)
    want, n = A.apply(data, model, [b"a"])
    b = capi.Batch(toy[1], 1000, 1000 * 160)
    try:
        m = capi.RecalModel(tables, 60, exclude=0x400)
        ap = capi.RecalApply(m, capi.DupGroups(header([b"a"])))
        empty = capi.Batch(toy[1], 10, 1000)
        assert L.bwams_recal_apply_batch(ap.h, empty.h, None) == ERR_ARG               # neither bam_run nor bam_upload
        empty.close()
        assert b.bam_upload(data) == len(recs)
        assert ap.batch(b) == n and b.bam_fetch()[0] == want
        assert b.bam_upload(data) == len(recs) and b.bam_sort() == len(recs)          # a sorted copy: both are rewritten
        before, _ = b.bam_sorted_fetch()
        assert sorted(bam.split_records(before)) == sorted(recs) and before != data
        assert ap.batch(b) == n
        after, _ = b.bam_sorted_fetch()
        assert after == A.apply(before, model, [b"a"])[0] and b.bam_fetch()[0] == want
        assert b.bam_sort() == len(recs) and b.bam_sorted_fetch()[0] == after         # returns at once, the same bytes
        ap.close()
    finally:
        b.close()


def test_aligned_batch_count_model_apply(toy):
    from test_gpu_markdup import _pe_chunk
    g, ix = toy
    t1, t2, _ = _pe_chunk(g, 300, 8)
    b = capi.Batch(ix, 1000, 1000 * 160)
    try:
        b.process_chunk2(t1, t2)
        b.bam_run()
        raw, _ = b.bam_fetch()
        counts = recal.Recal([len(g)], None)
        counts.set_ref(0, np.minimum(g, 4).astype(np.uint8))
        assert counts.add(raw) > 400
        model = A.Model(counts.tables, 500)
        want, n = A.apply(raw, model)
        assert n >= 600 and want != raw
        r = capi.Recal([len(g)])
        r.set_ref_index(ix)
        r.add_batch(b)
        m = capi.RecalModel.of(r)
        for what in range(4):
            assert np.array_equal(m.table(what), model.table(what)), what
        ap = capi.RecalApply(m)
        assert ap.batch(b) == n and b.bam_fetch()[0] == want
        for h in (ap, m, r):
            h.close()
    finally:
        b.close()
