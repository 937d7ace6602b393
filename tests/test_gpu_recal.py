"""Base recalibration tables on the GPU (csrc/recal.hip, csrc/api_recal.hip, host/bam_sort.cpp's bwams_sorter_set_recal) through the
C-ABI, compared exactly with bwams/recal.py's restatement of the rules and with the literal expectations of tests/test_recal.py.
Every add runs twice, through the LDS kernel and under BWAMS_RECAL_LDS=0 through the plain kernel; every comparison covers all four
tables and the text."""
import ctypes as C
import gzip

import numpy as np
import pytest

from bwams import bam, capi, recal, simulate
import test_recal as T
from test_depth import rec
from test_recal import rrec

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY = -3, -4
PIECE = 256 * 65280                                   # the sorter's deflate piece


@pytest.fixture(scope="module")
def toy():
    g = simulate.make_genome(400000, seed=61, repeat_frac=0.0)
    ix = capi.Index.build(g, 0)
    contigs = np.zeros(2, capi.CONTIG_DTYPE)
    contigs["offset"], contigs["len"] = [0, 150001], [150001, len(g) - 150001]           # an odd length in front of the seam
    ix.set_contigs(contigs)
    ix.set_contig_names(["chrA", "chrB"])
    yield g, ix
    ix.close()


@pytest.fixture
def way(monkeypatch):
    """way(lds): the kernel of the adds that follow (BWAMS_RECAL_LDS through bwams_debug_reload); the default again afterwards"""
    def set_(lds: bool):
        monkeypatch.setenv("BWAMS_RECAL_LDS", "1" if lds else "0")
        capi.debug_reload()
    yield set_
    monkeypatch.undo()
    capi.debug_reload()


def header(ids) -> bytes:
    return b"@HD\tVN:1.6\n" + b"".join(b"@RG\tID:%s\n" % i for i in ids)


def same(got: capi.Recal, want: recal.Recal):
    """all four tables and the text against the restatement"""
    for what in range(4):
        g, w = got.table(what), want.table(what)
        assert g.shape == w.shape and np.array_equal(g, w), (what, np.argwhere(g != w)[:8].tolist())
    assert got.text() == want.text()


def both(way, l_ref, ids, refs, known, adds, **opt):
    """the restatement, and a device handle per kernel, after the same reference, known-site calls and adds
    -> (want, LDS handle, plain handle).  ids: the read groups' IDs, or None for no groups table."""
    want = recal.Recal(l_ref, ids, **opt)
    for k, codes in enumerate(refs):
        want.set_ref(k, codes)
    for sites in known:
        want.add_known(sites)
    n, bases = [], 0
    for d in adds:
        n.append(want.add(d))
        bases = want.n_bases
    out = []
    for lds in (True, False):
        way(lds)
        groups = capi.DupGroups(header(ids)) if ids is not None else None
        got = capi.Recal(l_ref, groups, **opt)
        for k, codes in enumerate(refs):
            got.set_ref(k, codes)
        for sites in known:
            got.add_known(sites)
        assert [got.add_records(d) for d in adds] == n
        i = got.info()
        assert i["lds"] == int(lds) and i["n_counted"] == n[-1] and i["n_bases"] == bases
        assert i["n_records"] == len(bam.split_records(adds[-1])) and i["store_bytes"] == 4 * sum((x + 7) // 8 for x in l_ref)
        same(got, want)
        out.append(got)
    return want, out[0], out[1]


def close(*handles):
    for h in handles:
        h.close()


def random_ref(rng, n: int, n_frac: float = 0.0) -> np.ndarray:
    codes = rng.integers(0, 4, n).astype(np.uint8)
    codes[rng.random(n) < n_frac] = 4
    return codes


def read_of(rng, ref, pos: int, ops, err: float = 0.05, odd: float = 0.0):
    """SEQ codes (4-bit) for a CIGAR at pos: the reference under M, = and X but for mismatches, random elsewhere; `odd`: the share of
    codes 0 and 15"""
    seq = []
    x = pos
    for n, op in ops:
        if op in (0, 7, 8):
            for p in range(x, x + n):
                b = int(ref[p]) if 0 <= p < len(ref) and ref[p] < 4 and rng.random() >= err else int(rng.integers(0, 4))
                seq.append(1 << b)
        elif op in (1, 4):
            seq.extend(1 << int(b) for b in rng.integers(0, 4, n))
        if op in (0, 2, 3, 7, 8):
            x += n
    seq = np.array(seq, np.int64)
    at = rng.random(len(seq)) < odd
    seq[at] = rng.choice([0, 15], int(at.sum()))
    return seq


def random_record(rng, refs, ids, max_len: int = 150, odd: float = 0.02):
    refid = int(rng.integers(0, len(refs)))
    ref = refs[refid]
    ops = [(int(rng.integers(0, 4)), 5), (int(rng.integers(0, 6)), 4)]
    for _ in range(int(rng.integers(1, 5))):
        ops.append((int(rng.integers(1, max_len // 4)), int(rng.choice([0, 0, 7, 8]))))
        ops.append((int(rng.integers(0, 4)), int(rng.choice([1, 2, 3, 6]))))
    ops += [(int(rng.integers(0, 5)), 4), (int(rng.integers(0, 3)), 5)]
    pos = int(rng.integers(-1, max(len(ref) - 20, 1)))
    seq = read_of(rng, ref, pos, ops, odd=odd)
    qual = [int(q) for q in rng.choice([5, 6, 7, 20, 30, 37, 41, 93, 94, 200], len(seq))]
    if len(seq) and rng.random() < 0.03:
        qual[0] = 0xFF
    flag = int(rng.choice([0, 0x10, 0x41, 0x51, 0x81, 0x91, 0x80, 0x90, 0x800, 0x400, 0x4]))
    rg = None if ids is None or rng.random() < 0.1 else (b"nobody" if rng.random() < 0.1 else ids[int(rng.integers(0, len(ids)))])
    return rrec(refid, pos, ops, seq, qual, flag=flag, mapq=int(rng.choice([0, 1, 60])), rg=rg, aux=b"NMC\1", name=b"q")


def test_worked_example(way, toy):
    want, a, b = both(way, [8], [b"a"], [T.codes_of(T.EX_REF)], [], [b"".join(T.EX_RECS)], **T.EX_OPT)
    for got in (a, b):
        assert got.table(recal.RG).tolist() == [[16, 1], [0, 0]] and got.table(recal.CYCLE)[0, 30, 16].tolist() == [2, 1]
        assert got.table(recal.CONTEXT)[0, 30, 0].tolist() == [1, 1] and got.text() == T.EX_TEXT
        got.add_known([(0, 2, 3)])
        got.reset()                                                              # the reference and the flag stay
        assert got.add_records(b"".join(T.EX_RECS)) == 2 and got.text() == T.EX_TEXT_KNOWN
    close(a, b)
    # the same records from a batch, in HBM; its toy index has other lengths, the handle its own
    bt = capi.Batch(toy[1], 1000, 1000 * 160)
    try:
        assert bt.bam_upload(b"".join(T.EX_RECS)) == 2
        for lds in (True, False):
            way(lds)
            got = capi.Recal([8], capi.DupGroups(header([b"a"])), **T.EX_OPT)
            got.set_ref(0, T.codes_of(T.EX_REF))
            assert got.add_batch(bt) == 2 and got.text() == T.EX_TEXT
            got.close()
        empty = capi.Batch(toy[1], 10, 1000)
        h = capi.Recal([8])
        assert capi.lib().bwams_recal_add_batch(h.h, empty.h, None) == ERR_ARG     # neither bam_run nor bam_upload
        close(empty, h)
    finally:
        bt.close()


def test_lengths_strands_and_qualities(way):
    rng = np.random.default_rng(2)
    mc = 130
    ref = random_ref(rng, 400)
    recs = []
    for n in (1, 63, 64, 65, 128, 129, mc):
        for flag in (0, 0x10, 0x41, 0x51, 0x81, 0x91, 0x80, 0x90):               # both strands; first, last, and 0x80 without 0x1
            pos = int(rng.integers(0, 400 - n))
            q = [int(v) for v in rng.choice([5, 6, 93, 94, 255, 30], n)]           # min_baseq - 1, min_baseq, 93, and two that clamp
            recs.append(rrec(0, pos, [(n, 0)], read_of(rng, ref, pos, [(n, 0)]), q, flag=flag))
    recs.insert(3, rrec(0, 7, "64M", read_of(rng, ref, 7, [(64, 0)]), [0xFF] + [30] * 63))       # a first byte 0xFF: skipped
    recs.insert(9, rrec(0, 7, "5M", [1, 2, 4, 8, 1], [30, 0xFF, 94, 5, 6]))      # 0xFF behind the first byte clamps to 93
    want, a, b = both(way, [400], None, [ref], [], [b"".join(recs)], max_cycle=mc)
    cyc = want.table(recal.CYCLE)[0]
    assert cyc[93, mc + mc, 0] + cyc[30, mc + mc, 0] + cyc[6, mc + mc, 0] >= 1 and cyc[:, :mc, 0].sum() > 500      # cycle max_cycle; negative ones
    assert cyc[5].sum() == 0 and cyc[6, :, 0].sum() > 50 and cyc[93, :, 0].sum() > 200 and want.table(recal.RG)[0, 1] > 20
    long = rrec(0, 7, "131M", read_of(rng, ref, 7, [(131, 0)]))
    L = capi.lib()
    for got in (a, b):
        assert L.bwams_recal_add_records(got.h, recs[0] + long, len(recs[0] + long), None) == ERR_ARG
        assert L.bwams_last_error().decode() == "bwams_recal_add_records: record 1 is longer than max_cycle (cycle)"
        same(got, want)
    close(a, b)


def test_bases_contexts_and_cigars(way):
    rng = np.random.default_rng(3)
    ref = random_ref(rng, 300)
    A, C_, G, T_ = 1, 2, 4, 8
    hand = [rrec(0, 10, "6M", [A, 0, C_, 15, G, T_]),                            # codes 0 and 15 under the base and under its neighbour
            rrec(0, 10, "6M", [A, 0, C_, 15, G, T_], flag=0x10),
            rrec(0, 10, "2M3I2M", [A, C_, G, G, T_, A, C_]),                       # an insertion as the context neighbour
            rrec(0, 10, "2M3I2M", [A, C_, G, G, T_, A, C_], flag=0x10),
            rrec(0, 10, "3S4M", [T_, T_, G, A, C_, G, T_]),                        # a leading soft clip as the neighbour
            rrec(0, 10, "4M3S", [A, C_, G, T_, G, 15, A], flag=0x10),              # a trailing one, on the reverse strand
            rrec(0, 10, "2H1S2M1D1M2N1P2M1I1M2S3H", [A] * 10),                     # every op that only advances
            rrec(0, 10, "2=1X2=", [A, C_, G, T_, A]),
            rrec(0, 10, [(3, 9)], [A, C_, G], flag=0x4)]                            # op 9 in a filtered-out record: refused below
    recs = hand[:-1] + [random_record(rng, [ref], None) for _ in range(300)]
    want, a, b = both(way, [300], None, [ref], [], [b"".join(recs)], max_cycle=200)
    assert want.table(recal.CONTEXT)[..., 0].sum() < want.table(recal.QUAL)[..., 0].sum() - 50
    L = capi.lib()
    for data, at, why in ((recs[0] + hand[-1], 1, "has a CIGAR op code above 8 (op)"),
                          (recs[0] * 2 + rrec(0, 10, "2M1D2I1S", [A] * 4), 2, "has a CIGAR whose query length is not l_seq (length)")):
        for got in (a, b):
            assert L.bwams_recal_add_records(got.h, data, len(data), None) == ERR_ARG
            assert L.bwams_last_error().decode() == "bwams_recal_add_records: record %d %s" % (at, why)
            same(got, want)
    close(a, b)


def test_reference_positions(way):
    rng = np.random.default_rng(4)
    l_ref = [37, 0, 64, 1, 9, 130]                                               # odd and even lengths back to back, one of length 0
    refs = [random_ref(rng, n, 0.1) for n in l_ref]                               # with N
    recs = []
    for r, n in enumerate(l_ref):
        if n == 0:
            recs.append(rrec(r, 0, "4M", [1, 2, 4, 8]))
            continue
        for pos, length in ((-1, min(n + 3, 40)), (0, n), (max(n - 5, 0), 12), (n - 1, 1), (n - 1, 9)):       # over position 0 and over the end
            ops = [(length, 0)]
            recs.append(rrec(r, pos, ops, read_of(rng, refs[r], pos, ops), flag=int(rng.choice([0, 0x10]))))
    known = [[(0, 36, 37), (2, 0, 1), (5, 7, 9)], [(2, 63, 64), (4, 0, 9)]]
    want, a, b = both(way, l_ref, None, refs, known, [b"".join(recs)], max_cycle=130)
    assert want.table(recal.RG)[0, 0] > 200 and want.table(recal.RG)[0, 1] > 5
    close(a, b)


def test_known_sites(way):
    rng = np.random.default_rng(5)
    n = 131
    ref = random_ref(rng, n)
    ops = [(n, 0)]
    recs = [rrec(0, 0, ops, read_of(rng, ref, 0, ops, err=0.5), q) for q in (20, 30)]      # a cycle per position: a flag off by one shows
    edges = [(0, p, p + 1) for p in (0, 1, 31, 32, 63, 64, n - 1)]                 # word and byte edges of the store, and the last position
    want, a, b = both(way, [n], None, [ref], [edges], [b"".join(recs)], max_cycle=n)
    assert want.table(recal.RG)[0, 0] == 2 * (n - 7)
    close(a, b)
    spans = [[(0, 60, 70), (0, 3, 40), (0, 30, 35), (0, 3, 4)], [(0, 100, 131), (0, 64, 72)]]      # unsorted, overlapping, two calls
    want, a, b = both(way, [n], None, [ref], spans, [b"".join(recs)], max_cycle=n)
    assert want.table(recal.RG)[0, 0] == 2 * (3 + 20 + 28)
    L = capi.lib()
    bad = np.array([(0, 80, 90), (0, 90, 132), (0, 5, 5)], capi.RECAL_SITE_DTYPE)
    for got in (a, b):
        got.reset()
        for sites in (bad, bad[[0, 2]], np.array([(1, 0, 1)], capi.RECAL_SITE_DTYPE), np.array([(0, -1, 1)], capi.RECAL_SITE_DTYPE)):
            assert L.bwams_recal_add_known(got.h, sites.ctypes.data_as(C.c_void_p), len(sites)) == ERR_ARG
        assert L.bwams_last_error().decode() == "bwams_recal_add_known: interval 0 is not 0 <= beg < end <= l_ref[ref]"
        assert L.bwams_recal_add_known(got.h, bad.ctypes.data_as(C.c_void_p), 3) == ERR_ARG
        assert L.bwams_last_error().decode() == "bwams_recal_add_known: interval 1 is not 0 <= beg < end <= l_ref[ref]"
        assert got.add_records(b"".join(recs)) == 2
        same(got, want)                                                          # the flags as they were: 80..89 not set
    close(a, b)


def test_read_groups(way):
    rng = np.random.default_rng(6)
    ref = random_ref(rng, 500)

    def reads(n, pick):
        out = []
        for k in range(n):
            pos, ops = int(rng.integers(0, 430)), [(int(rng.integers(20, 70)), 0)]
            out.append(rrec(0, pos, ops, read_of(rng, ref, pos, ops), int(rng.choice([20, 30])), flag=int(rng.choice([0, 0x10, 0x91])),
                            rg=pick(k), aux=b"XAAx"))
        return out
    for ids in (None, [b"solo"], [b"b", b"a", b"ab"]):                           # none, one and three; IDs not in byte order
        names = [None, b"zz"] + (ids or [b"x"])                                   # no RG, an unknown RG, and every known one
        want, a, b = both(way, [500], ids, [ref], [], [b"".join(reads(120, lambda k: names[k % len(names)]))])
        rg = want.table(recal.RG)
        assert (rg[:, 0] > 0).all() and rg.shape[0] == (len(ids) if ids else 0) + 1
        close(a, b)
    many = [b"g%03d" % k for k in range(40)]                                     # a workgroup changes group many times; group 7 fills two slices
    recs = reads(1500, lambda k: many[int(rng.integers(0, 40))]) + reads(1100, lambda k: many[7])
    order = rng.permutation(len(recs))
    want, a, b = both(way, [500], many, [ref], [], [b"".join(recs[k] for k in order)])
    assert (want.table(recal.RG)[:40, 0] > 0).all() and a.info()["slice"] < 1100
    L = capi.lib()
    broken = rrec(0, 5, "3M", [1, 2, 4], rg=b"g001", aux=b"XXZabc")              # a Z field without its NUL
    data = recs[0] + recs[1] + broken
    for got in (a, b):
        assert L.bwams_recal_add_records(got.h, data, len(data), None) == ERR_ARG
        assert L.bwams_last_error().decode() == "bwams_recal_add_records: record 2 has aux fields that do not chain to its end (aux)"
        same(got, want)
    close(a, b)
    for lds in (True, False):                                                    # without a table the aux fields are not read
        way(lds)
        got = capi.Recal([500])
        assert got.add_records(data) == 3
        got.close()


def test_random_records(way):
    rng = np.random.default_rng(7)
    l_ref = [900, 333, 2000]
    refs = [random_ref(rng, n, 0.02) for n in l_ref]
    ids = [b"r1", b"r2", b"r3"]
    recs = [random_record(rng, refs, ids) for _ in range(3000)]
    known = [[(int(r), int(p), int(p) + int(w)) for r, p, w in zip(rng.integers(0, 3, 40), rng.integers(0, 300, 40), rng.integers(1, 30, 40))]]
    parts = [b"".join(recs[:700]), b"", b"".join(recs[700:701]), b"".join(recs[701:])]
    want, a, b = both(way, l_ref, ids, refs, known, parts, max_cycle=200)
    whole = recal.Recal(l_ref, ids, max_cycle=200)
    for k, codes in enumerate(refs):
        whole.set_ref(k, codes)
    whole.add_known(known[0])
    whole.add(b"".join(recs))
    rg = whole.table(recal.RG)
    assert (rg[:, 0] > 5000).all() and (rg[:, 1] > 200).all() and whole.table(recal.CYCLE)[:, :, :200, 0].sum() > 5000
    for got in (a, b):
        same(got, whole)                                                         # several adds are one add
        got.reset()
        for d in reversed(parts):                                                # in the other order
            got.add_records(d)
        same(got, whole)
    close(a, b)


@pytest.mark.parametrize("tag,data,at,why,groups", T.refusals(), ids=[r[0] for r in T.refusals()])
def test_refusals(way, tag, data, at, why, groups):
    L = capi.lib()
    text = {"op": "has a CIGAR op code above 8 (op)", "length": "has a CIGAR whose query length is not l_seq (length)",
            "bounds": "ends inside its SEQ or QUAL (bounds)", "cycle": "is longer than max_cycle (cycle)",
            "aux": "has aux fields that do not chain to its end (aux)"}[why]
    want = recal.Recal([100], [b"a"] if groups else None, max_cycle=20)
    want.set_ref(0, np.zeros(100, np.uint8))
    want.add(T.GOOD * 3)
    for lds in (True, False):
        way(lds)
        got = capi.Recal([100], capi.DupGroups(T.HEADER) if groups else None, max_cycle=20)
        got.set_ref(0, np.zeros(100, np.uint8))
        assert got.add_records(T.GOOD * 3) == 3
        n = C.c_int64(-1)
        assert L.bwams_recal_add_records(got.h, data, len(data), C.byref(n)) == ERR_ARG
        assert L.bwams_last_error().decode() == "bwams_recal_add_records: record %d %s" % (at, text)
        same(got, want)                                                          # a refused call adds nothing
        got.close()


def test_state_and_arguments(way, toy):
    L = capi.lib()
    g, ix = toy
    l_ref = [150001, len(g) - 150001]
    by_ref = [np.minimum(g[:150001], 4).astype(np.uint8), np.minimum(g[150001:], 4).astype(np.uint8)]
    rng = np.random.default_rng(8)
    recs = []
    for refid, pos in ((0, 0), (0, 149990), (0, 149941), (1, 0), (1, 7), (1, l_ref[1] - 60), (0, 75000)):      # both sides of the seam
        ops = [(60, 0)]
        recs.append(rrec(refid, pos, ops, read_of(rng, by_ref[refid], pos, ops, err=0.1)))
    data = b"".join(recs)
    want = recal.Recal(l_ref, None)
    for k in range(2):
        want.set_ref(k, by_ref[k])
    want.add_known([(0, 150000, 150001), (1, 0, 1)])
    want.add(data)
    assert want.table(recal.RG)[0, 0] > 350 and 10 < want.table(recal.RG)[0, 1] < 100
    for lds in (True, False):
        way(lds)
        a, b = capi.Recal(l_ref), capi.Recal(l_ref)
        a.add_known([(0, 150000, 150001), (1, 0, 1)])                            # before the reference: neither touches the other
        a.set_ref_index(ix)
        for k in range(2):
            b.set_ref(k, by_ref[k])
        b.add_known([(0, 150000, 150001), (1, 0, 1)])
        for got in (a, b):
            assert got.add_records(data) == len(recs)
            same(got, want)
        close(a, b)
    wrong = capi.Recal([150001, 5])
    assert L.bwams_recal_set_ref_index(wrong.h, ix.h) == ERR_ARG and L.bwams_recal_set_ref_index(wrong.h, None) == ERR_ARG
    codes = np.zeros(5, np.uint8)
    codes[3] = 5
    assert L.bwams_recal_set_ref(wrong.h, 1, codes.ctypes.data_as(C.c_void_p)) == ERR_ARG
    assert L.bwams_last_error().decode() == "bwams_recal_set_ref: code 3 is above 4"
    assert L.bwams_recal_set_ref(wrong.h, 2, codes.ctypes.data_as(C.c_void_p)) == ERR_ARG
    wrong.close()
    a = capi.Recal([8], capi.DupGroups(header([b"a"])), **T.EX_OPT)
    a.set_ref(0, T.codes_of(T.EX_REF))
    a.add_records(b"".join(T.EX_RECS))
    n = C.c_int64(0)
    buf = np.zeros(20000, np.int64)
    vp = buf.ctypes.data_as(C.c_void_p)
    for what, size in enumerate([2 * 2, 2 * 94 * 2, 2 * 94 * 21 * 2, 2 * 94 * 16 * 2]):
        assert L.bwams_recal_table(a.h, what, None, 0, C.byref(n)) == 0 and n.value == size         # NULL: the size
        assert L.bwams_recal_table(a.h, what, vp, size - 1, C.byref(n)) == ERR_CAPACITY and n.value == size
        assert L.bwams_recal_table(a.h, what, vp, size, None) == 0 and np.array_equal(buf[:size], T.example().table(what).reshape(-1))
    assert L.bwams_recal_table(a.h, 4, vp, 20000, C.byref(n)) == ERR_ARG and L.bwams_recal_table(a.h, -1, vp, 20000, C.byref(n)) == ERR_ARG
    assert L.bwams_recal_table(a.h, 0, vp, -1, C.byref(n)) == ERR_ARG and L.bwams_recal_table(None, 0, vp, 20000, C.byref(n)) == ERR_ARG
    out = C.create_string_buffer(4096)
    gh = a.groups.h
    assert L.bwams_recal_text(a.h, gh, None, 0, C.byref(n)) == ERR_CAPACITY and n.value == len(T.EX_TEXT)
    assert L.bwams_recal_text(a.h, gh, out, len(T.EX_TEXT) - 1, C.byref(n)) == ERR_CAPACITY and n.value == len(T.EX_TEXT)
    assert L.bwams_recal_text(a.h, gh, out, len(T.EX_TEXT), C.byref(n)) == 0 and out.raw[:n.value].decode() == T.EX_TEXT
    assert L.bwams_recal_text(a.h, None, out, 4096, C.byref(n)) == ERR_ARG and L.bwams_recal_text(None, gh, out, 4096, C.byref(n)) == ERR_ARG
    assert a.groups.rg_id(0) == "a" and a.groups.rg_id(1) is None and a.groups.rg_id(-1) is None
    assert L.bwams_recal_info(a.h, None) == ERR_ARG and L.bwams_recal_reset(None) == ERR_ARG
    cut = T.GOOD[:-1]
    assert L.bwams_recal_add_records(a.h, cut, len(cut), None) == ERR_ARG        # the chain, as bwams_bam_upload checks it
    assert L.bwams_recal_add_records(a.h, None, 5, None) == ERR_ARG
    a.close()
    h = C.c_void_p()
    lens = np.array([8], np.int32)
    lp = lens.ctypes.data_as(C.c_void_p)
    for o in (capi.RecalOpt(0x10000, 1, 6, 500, 0), capi.RecalOpt(0x704, 1, -1, 500, 0), capi.RecalOpt(0x704, 1, 94, 500, 0),
              capi.RecalOpt(0x704, 1, 6, 0, 0), capi.RecalOpt(0x704, 1, 6, 500, 1)):
        assert L.bwams_recal_open(0, lp, 1, None, C.byref(o), C.byref(h)) == ERR_ARG
    neg = np.array([8, -1], np.int32)
    assert L.bwams_recal_open(0, neg.ctypes.data_as(C.c_void_p), 2, None, None, C.byref(h)) == ERR_ARG
    assert L.bwams_recal_open(0, lp, 1, None, None, None) == ERR_ARG and L.bwams_recal_open(0, lp, -1, None, None, C.byref(h)) == ERR_ARG
    assert L.bwams_recal_open(99, lp, 1, None, None, C.byref(h)) != 0            # no such device
    assert L.bwams_recal_open(0, lp, 1, None, None, C.byref(h)) == 0             # NULL: the defaults
    assert L.bwams_recal_table(h, recal.CYCLE, None, 0, C.byref(n)) == 0 and n.value == 94 * 1001 * 2
    assert L.bwams_recal_close(h) == 0 and L.bwams_recal_close(None) == 0


def test_from_a_real_batch(way, toy):
    from test_gpu_markdup import _pe_chunk
    g, ix = toy
    l_ref = [150001, len(g) - 150001]
    t1, t2, _ = _pe_chunk(g, 1200, 8)
    b = capi.Batch(ix, 4000, 4000 * 160)
    try:
        b.process_chunk2(t1, t2)
        b.bam_run()
        raw, _ = b.bam_fetch()
        want = recal.Recal(l_ref, None)
        want.set_ref(0, np.minimum(g[:150001], 4).astype(np.uint8))
        want.set_ref(1, np.minimum(g[150001:], 4).astype(np.uint8))
        n = want.add(raw)
        rg = want.table(recal.RG)[0]
        assert n > 2000 and rg[0] > 100000 and 0 < rg[1] < rg[0] // 10 and want.table(recal.CYCLE)[0, :, :500, 0].sum() > 100000
        for lds in (True, False):
            way(lds)
            got = capi.Recal(l_ref)
            got.set_ref_index(ix)
            assert got.add_batch(b) == n
            same(got, want)
            got.close()
    finally:
        b.close()


def _sorter(tmp_path, tag, ix, hdr, runs, r=None, q=None, p=None, d=None):
    path = str(tmp_path / ("%s.bam" % tag))
    s = capi.Sorter(path, 0, hdr, markdup=True)
    b = capi.Batch(ix, 1000, 1000 * 160)
    try:
        for h, set_ in ((r, s.set_recal), (q, s.set_qc), (p, s.set_pileup), (d, s.set_depth)):
            if h is not None:
                set_(h)
        for k, run in enumerate(runs):
            b.bam_upload(run)
            s.put_batch(k, b)
            if k == 0 and r is not None:
                assert capi.lib().bwams_sorter_set_recal(s.h, r.h) == ERR_ARG  # after a put
                assert capi.lib().bwams_last_error().decode() == "bwams_sorter_set_recal: called after the sorter's first put"
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
    refs = [random_ref(rng, n) for n in l_ref]
    hdr = bam.header_block(b"@HD\tVN:1.6\tSO:coordinate\n", [b"s0", b"s1"], l_ref)
    runs, k = [], 0
    for put in range(3):
        recs = []
        for _ in range(600):
            recs.append(_fragment(k, int(rng.integers(0, 2)), int(rng.integers(0, 2800)), flag=16 * int(rng.integers(0, 2))))
            k += 1
        runs.append(recs)
    runs[0].insert(5, _fragment(90000, 0, 4000, qual=40))                       # kept: the best of its place ...
    runs[2].insert(9, _fragment(90001, 0, 4000, qual=20))                       # ... its duplicate comes two puts later
    runs[1].insert(3, _fragment(90002, 1, 2890, flag=0x400))                    # a stale mark on a record that is no duplicate: cleared
    runs = [b"".join(x) for x in runs]

    def handle():
        h = capi.Recal(l_ref)
        for r_, codes in enumerate(refs):
            h.set_ref(r_, codes)
        h.add_known([(0, 4000, 4010)])
        return h
    r1, r4 = handle(), handle()
    q4, p4, d4 = capi.Qc(exclude=0xD00), capi.Pileup(l_ref), capi.Depth(l_ref)
    data0, x0, st0 = _sorter(tmp_path, "plain", ix, hdr, runs)
    data1, x1, st1 = _sorter(tmp_path, "recal", ix, hdr, runs, r=r1)
    data4, x4, _ = _sorter(tmp_path, "all", ix, hdr, runs, r=r4, q=q4, p=p4, d=d4)          # all four handles on one sorter
    assert data0 == data1 == data4 and x0 == x1 == x4                           # the file and its index do not know about the handles
    written = gzip.decompress(data0)[len(hdr):]
    want = recal.Recal(l_ref)
    for r_, codes in enumerate(refs):
        want.set_ref(r_, codes)
    want.add_known([(0, 4000, 4010)])
    n = want.add(written)
    assert st1.dup.records_marked >= 1 and n == st1.records - st1.dup.records_marked and st1.records == 1803      # duplicates are not counted
    for h in (r1, r4):
        same(h, want)
    asgiven = recal.Recal(l_ref)
    assert asgiven.add(b"".join(runs)) == 1802                                  # the stale mark; the real duplicate was not marked yet
    assert q4.summary()[0][0, 0] == 1803 and d4.finish().fetch(1).sum() == p4.fetch(1)[:, :8].sum()
    L = capi.lib()
    s = capi.Sorter(str(tmp_path / "args.bam"), 0, hdr)
    assert L.bwams_sorter_set_recal(s.h, None) == ERR_ARG and L.bwams_sorter_set_recal(None, r1.h) == ERR_ARG
    other = capi.Recal([5000, 3001])
    assert L.bwams_sorter_set_recal(s.h, other.h) == ERR_ARG                    # other reference lengths
    assert L.bwams_last_error().decode() == "bwams_sorter_set_recal: the recalibration handle's reference lengths are not the sorter header's"
    n_dev = C.c_int(0)
    L.bwams_device_count(C.byref(n_dev))
    if n_dev.value > 1:                                                         # with one GPU this case does not run
        far = capi.Recal(l_ref, device=1)
        assert L.bwams_sorter_set_recal(s.h, far.h) == ERR_ARG                  # another device
        far.close()
    assert L.bwams_sorter_set_recal(s.h, r1.h) == 0
    s.close()
    close(r1, r4, q4, p4, d4, other)


def test_sorter_record_across_pieces(tmp_path, toy):
    """just over one deflate piece of records: one straddles the cut and is counted once, with the flag the merge gave it.  Every
    record is 100M of A with quality 30 on the forward strand over a reference of A, so every cell has a closed form."""
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
    r = capi.Recal(l_ref)
    r.set_ref(0, np.zeros(200000, np.uint8))
    data, _, st = _sorter(tmp_path, "cut", ix, hdr, runs, r=r)
    assert st.records == n and st.dup.records_marked == 0
    assert r.table(recal.RG).tolist() == [[100 * n, 0]] and r.table(recal.QUAL)[0, 30].tolist() == [100 * n, 0]
    cyc, ctx = r.table(recal.CYCLE), r.table(recal.CONTEXT)
    assert (cyc[0, 30, 501:601, 0] == n).all() and cyc.sum() == 100 * n and ctx[0, 30, 0].tolist() == [99 * n, 0] and ctx.sum() == 99 * n
    r.close()
