"""How a task slot of the packed banded-SW kernel gets its next task (csrc/bsw_extend.hip, bsw_pk_kernel): a wave stages the
sixteen descriptors of a ticket at once, a refilling quad fetches its own from the staging lanes, and the whole wave writes the
slot's row -1 and query, four columns per lane.  The edges of exactly that: tickets that are not full and ticket boundaries met
mid-wave, query lengths around the four-column granule and the classes, many slots refilling in one iteration, queries and
targets at the two ends of the uploaded buffers, and the in-place form with dir = -1 / +1 through the extension stage.  The
oracle is loader.bsw_pairs (the regions: loader.chain2aln); every test runs with BWAMS_BSW_PK=1 and =0."""
import numpy as np
import pytest

from bwams import capi, fmindex, simulate
from oracle import loader
from util import assert_pairs_equal, bsw_class, bsw_sw_opt, make_task_pool, mutate, pack_pairs, toy

pytestmark = pytest.mark.gpu

IN_FIELDS = ("idr", "idq", "id", "len1", "len2", "h0", "seqid", "regid")
W = 100
GRANULE_QLENS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 63, 64, 95, 96, 143, 144, 191)


@pytest.fixture(scope="module")
def ix():
    capi.lib()
    _, idx = toy(20000)
    h = capi.Index.from_host(idx, 0)
    yield h
    h.close()


@pytest.fixture(params=["1", "0"], ids=["pk", "qwin"])
def knob(request, monkeypatch):
    monkeypatch.setenv("BWAMS_BSW_PK", request.param)
    capi.debug_reload()                                    # the switches are read once: say that it changed
    return request.param


def _opts():
    return bsw_sw_opt(loader), bsw_sw_opt(capi)


def _run(b, pairs, ref, qer, want, cells, what):
    b.bsw_upload(pairs, ref, qer)
    b.bsw_run(W, _opts()[1])
    got = b.bsw_fetch()
    assert_pairs_equal(got, want, what)
    assert b.stats().bsw_cells == cells, what
    for f in IN_FIELDS:
        assert np.array_equal(got[f], pairs[f]), (what, f)


def _check(ix, pairs, ref, qer, what):
    want, cells = loader.bsw_pairs(pairs, ref, qer, W, _opts()[0])
    b = capi.Batch(ix, 8, 1200)
    try:
        _run(b, pairs, ref, qer, want, cells, what)
    finally:
        b.close()
    return want


def _second_ticket_tasks():
    """More tasks of one class than the first tickets of every wave of its launch cover (tests/test_gpu_bsw.py, refill_set): a
    launch starts at most 4 * 8 waves per CU and a ticket is sixteen tasks."""
    import torch
    return 512 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def pool():
    """300 distinct tasks of one class (queries of 32-63 bases, targets of up to 300) with the oracle's answer and cells of each"""
    q, t, h = make_task_pool(300, 32, 63, seed=700, tlen_max=300)
    pairs, ref, qer = pack_pairs(q, t, h)
    assert (bsw_class(pairs["len2"], pairs["h0"], 1) == 1).all()
    oo = _opts()[0]
    want, total = loader.bsw_pairs(pairs, ref, qer, W, oo)
    cells = np.array([loader.bsw_pairs(pairs[i:i + 1], ref, qer, W, oo)[1] for i in range(len(pairs))], np.int64)
    assert cells.sum() == total
    return dict(pairs=pairs, ref=ref, qer=qer, want=want, cells=cells)


def _tiled(ix, pool, sel, what):
    """the pool's tasks sel[0], sel[1], ... as one launch"""
    big = np.ascontiguousarray(pool["pairs"][sel])
    big["id"] = np.arange(len(sel))
    b = capi.Batch(ix, 8, 1200)
    try:
        _run(b, big, pool["ref"], pool["qer"], pool["want"][sel], int(pool["cells"][sel].sum()), what)
    finally:
        b.close()


# ---- ticket edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 33, "16k+1"])
def test_ticket_edges(ix, knob, pool, n):
    """Fewer tasks than a wave has slots, a last ticket that is not full, and (16 k + 1, with k large enough that waves take
    further tickets) ticket boundaries met while other slots of the wave are mid-task, the very last ticket holding one task."""
    if n == "16k+1":
        n = 16 * (_second_ticket_tasks() // 16 + 40) + 1
        assert n % 16 == 1 and n > _second_ticket_tasks()
    sel = np.arange(n) % len(pool["pairs"])
    _tiled(ix, pool, sel, f"{n} tasks of one class, BWAMS_BSW_PK={knob}")


# ---- granule edges -------------------------------------------------------------------------------------------------------
def test_granule_edges(ix, knob):
    """Query lengths around the four-column granule a lane writes and on both sides of every class edge, each with targets of
    0 (the slot is refilled but never runs), 1 and many bases; N in queries and targets."""
    rng = np.random.default_rng(701)
    qs, ts, hs = [], [], []
    for ql in GRANULE_QLENS:
        for rep in range(3):
            q = rng.integers(0, 4, size=ql, dtype=np.uint8)
            if rep == 2:
                q[rng.integers(0, ql)] = 4
            tail = rng.integers(0, 4, size=40, dtype=np.uint8)
            for t in (q[:0], q[:1], np.concatenate([q, tail]), np.concatenate([mutate(rng, q, 0.08), tail])):
                qs.append(q); ts.append(t); hs.append(int(rng.integers(1, 120)))
    pairs, ref, qer = pack_pairs(qs, ts, hs)
    assert set(pairs["len2"]) == set(GRANULE_QLENS) and (pairs["len1"] == 0).sum() >= len(GRANULE_QLENS)
    assert set(np.unique(bsw_class(pairs["len2"], pairs["h0"], 1))) == set(range(5))
    want = _check(ix, pairs, ref, qer, f"granule edges, BWAMS_BSW_PK={knob}")
    assert (want["score"][pairs["len1"] > 1] > pairs["h0"][pairs["len1"] > 1]).any()


# ---- several slots refilling in the same iteration -----------------------------------------------------------------------
def test_slots_refill_together(ix, knob, pool):
    """Blocks of 64 copies of one task (a ticket of sixteen copies ends on one row: sixteen slots refill in the same iteration),
    then distinct tasks, then tasks that end at row 0 (an unrelated target: the first row's maximum is 0) or have no target at
    all — tiled until the waves take further tickets."""
    p = pool["pairs"]
    row0 = np.flatnonzero((pool["want"]["tle"] == 0) & (p["len1"] > 0))
    empty = np.flatnonzero(p["len1"] == 0)
    long_ = np.flatnonzero(pool["want"]["tle"] > 30)
    assert len(row0) >= 2 and len(empty) >= 2 and len(long_) >= 8
    rng = np.random.default_rng(702)
    blocks = []
    for k in range(8):
        blocks += [np.full(64, long_[k]), rng.permutation(len(p))[:48], np.resize(row0, 16), np.resize(empty, 8), np.resize(row0, 8)]
    block = np.concatenate(blocks)
    n = _second_ticket_tasks() + 64 * len(block)
    _tiled(ix, pool, np.resize(block, n), f"slots refilling together, BWAMS_BSW_PK={knob}")


# ---- placement at the buffer ends ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ql", [1, 2, 3, 5, 8, 31, 64, 191])
def test_buffer_ends(ix, knob, ql):
    """The first task's query and target are the first bytes of the uploaded buffers, the last task's are their last bytes
    (pack_pairs' spare byte taken off)."""
    rng = np.random.default_rng(703 + ql)
    qs, ts, hs = [], [], []
    for k in range(20):
        q = rng.integers(0, 4, size=ql if k in (0, 19) else int(rng.integers(1, 192)), dtype=np.uint8)
        t = np.concatenate([mutate(rng, q, 0.05), rng.integers(0, 4, size=30, dtype=np.uint8)])
        qs.append(q); ts.append(t); hs.append(int(rng.integers(1, 120)))
    pairs, ref, qer = pack_pairs(qs, ts, hs)
    ref, qer = np.ascontiguousarray(ref[:-1]), np.ascontiguousarray(qer[:-1])
    assert pairs["idq"][0] == 0 and pairs["idr"][0] == 0 and pairs["len2"][0] == ql
    assert pairs["idq"][-1] + pairs["len2"][-1] == len(qer) and pairs["len2"][-1] == ql
    assert pairs["idr"][-1] + pairs["len1"][-1] == len(ref) and pairs["len1"][-1] > 0
    _check(ix, pairs, ref, qer, f"buffer ends, qlen {ql}, BWAMS_BSW_PK={knob}")


# ---- the in-place form, dir = -1 and +1, through the extension stage -----------------------------------------------------
REG_FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "sub", "csub", "w", "seedcov", "seedlen0")


@pytest.fixture(scope="module")
def edge_chunk():
    """Reads copied from a repeat-free genome with one mismatch d bases from an end, d = 0 (none) .. 4: the seed then starts at
    read offset d + 1 (the left task's query is those bases, read backwards in the in-place form) or ends that far from the
    read's end.  Offset 0 / the full length are the reads without a mismatch.  The chunk's first and last read are among them,
    on both strands."""
    capi.lib()
    g = simulate.make_genome(60000, seed=33, repeat_frac=0.0)
    idx = fmindex.build_fmindex(g)
    rng = np.random.default_rng(704)
    L = 120
    edge = []
    for d in range(0, 5):
        for at_start in (True, False):
            for rev in (False, True):
                st = int(rng.integers(100, len(g) - 300))
                r = g[st:st + L].copy()
                if d:
                    p = d - 1 if at_start else L - d
                    r[p] = (r[p] + 1) & 3
                edge.append(simulate.revcomp(r) if rev else r)
    plain, _, _ = simulate.make_reads(g, 200, seed=35)
    reads = edge[:10] + list(plain) + edge[10:]
    enc, cum = simulate.flatten_reads(reads)
    o = loader.OracleFMI(idx)
    sm = o.collect_smem(enc, cum)
    coord, off = o.sa_lookup(sm)
    l_pac = len(g)
    ref = np.concatenate([g, (3 - g[::-1]).astype(np.uint8)])
    chains, seeds, chain_off = loader.chain_seeds(sm, coord, off, cum, l_pac)
    wregs, wreg_off, wseeds, tasks = loader.chain2aln(chains, seeds, chain_off, enc, cum, ref, l_pac, want_tasks=True)
    # the oracle's tasks have the short queries the reads were built for (a query of 0 bases is no task)
    assert set(range(1, 5)) <= set(tasks["left"]["len2"]) and set(range(1, 5)) <= set(tasks["right"]["len2"])
    first, last = slice(wreg_off[0], wreg_off[1]), slice(wreg_off[-2], wreg_off[-1])
    assert wregs["score"][first].max() >= L - 10 and wregs["score"][last].max() >= L - 10
    ixh = capi.Index.from_host(idx, 0)
    yield dict(ix=ixh, enc=enc, cum=cum, n_sm=len(sm), n_sa=len(coord), wregs=wregs, wreg_off=wreg_off, aln=wseeds["aln"])
    ixh.close()


@pytest.mark.parametrize("inplace", ["1", "0"])
def test_inplace_short_queries(edge_chunk, knob, monkeypatch, inplace):
    monkeypatch.setenv("BWAMS_EXT_INPLACE", inplace)
    capi.debug_reload()
    c = edge_chunk
    b = capi.Batch(c["ix"], len(c["cum"]) - 1, int(c["cum"][-1]), max_smem=c["n_sm"] + 4096, max_sa=c["n_sa"] + 4096)
    try:
        b.seed_upload(c["enc"], c["cum"])
        b.seed_run(with_sa=True)
        gopt = capi.default_mem_opt()
        b.chain_run(gopt)
        n = b.extend_run(gopt)
        regs, reg_off, aln = b.extend_fetch()
    finally:
        b.close()
    wregs = c["wregs"]
    assert n == len(wregs) and np.array_equal(reg_off, c["wreg_off"]) and np.array_equal(aln, c["aln"])
    purged = (wregs["qb"] == -1) & (wregs["qe"] == -1)
    assert np.array_equal((regs["qb"] == -1) & (regs["qe"] == -1), purged)
    for f in REG_FIELDS:
        assert np.array_equal(regs[f][~purged], wregs[f][~purged]), (f, inplace, knob)
