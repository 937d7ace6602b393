"""Banded-SW extension on the GPU at the limits of each of its three kernels, against the scalar oracle (loader.bsw_pairs).

launch_bsw (csrc/bsw_extend.hip) sorts tasks into six classes and runs bsw_pk_kernel (16 tasks per wave, 16-bit lanes) or
bsw_qwin_kernel (8 tasks per wave, 14-bit packed H/E) on classes 0-4 and bsw_kernel (one task per wave) on class 5.  Every
test runs with BWAMS_BSW_PK=1 (the packed kernel where the scoring allows it) and BWAMS_BSW_PK=0 (the eight-task kernel), and
checks the six outputs bit for bit, the DP cell count, and that the input fields come back unchanged."""
import numpy as np
import pytest

from bwams import capi
from oracle import loader
from util import (BSW_LIMIT as LIMIT, BSW_SCORING_EDGES, BSW_WIDE_W, assert_pairs_equal, bsw_class, bsw_class_edge_tasks, bsw_n_run_tasks,
                  bsw_score_limit_tasks, bsw_scoring_edge_tasks, bsw_sw_opt, bsw_wide_band_tasks, make_pairs, make_task_pool, mutate, pack_pairs,
                  toy)

pytestmark = pytest.mark.gpu

IN_FIELDS = ("idr", "idq", "id", "len1", "len2", "h0", "seqid", "regid")
ERR_UNSUPPORTED = -6
MAX_QLEN = 18196                 # the longest query one wave's LDS row holds (160 KiB)


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


def _opts(**kw):
    """the same scoring for the oracle and for the library"""
    return bsw_sw_opt(loader, **kw), bsw_sw_opt(capi, **kw)


def _check(b, pairs, ref, qer, w, opts=None, what=""):
    """Batch.bsw against the oracle: outputs, cells, inputs untouched.  Returns the oracle's answers."""
    if isinstance(b, capi.Index):                          # on a batch of its own
        b = capi.Batch(b, 8, 1200)
        try:
            return _check(b, pairs, ref, qer, w, opts, what)
        finally:
            b.close()
    oo, go = opts or _opts()
    want, cells = loader.bsw_pairs(pairs, ref, qer, w, oo)
    got = b.bsw(pairs, ref, qer, w, go)
    assert_pairs_equal(got, want, what)
    assert b.stats().bsw_cells == cells, what
    for f in IN_FIELDS:
        assert np.array_equal(got[f], pairs[f]), (what, f)
    return want


def _oracle_per_task(pairs, ref, qer, w, oo):
    """Oracle answers and DP cells of every task (cells per task, so that a tiled set's total is a sum by index)."""
    want, total = loader.bsw_pairs(pairs, ref, qer, w, oo)
    cells = np.array([loader.bsw_pairs(pairs[i:i + 1], ref, qer, w, oo)[1] for i in range(len(pairs))], np.int64)
    assert cells.sum() == total
    return want, cells


# ---- task refill under load ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refill_set():
    """A pool of distinct tasks per class, its oracle answers, and a tiling of it large enough that in every packed-class launch
    some wave must take a second ticket of tasks: its slots then refill one by one while the others carry on."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    qs, ts, hs = [], [], []
    for c, (lo, hi) in enumerate(((1, 31), (32, 63), (64, 95), (96, 143), (144, 191), (192, 320))):
        q, t, h = make_task_pool(2500 if c < 5 else 400, lo, hi, seed=100 + c)
        qs += q; ts += t; hs.append(h)
    h0 = np.concatenate(hs)
    ql = np.array([len(q) for q in qs])
    # h0 near the bound: scores up to 2^14 - 1 in the packed classes, and class 5 by score rather than length.  The first column
    # stays positive for thousands of rows, so these tasks live for their whole target
    near = np.random.default_rng(99).choice(np.flatnonzero(ql <= 191), size=200, replace=False)
    h0[near[:100]] = LIMIT - 1 - ql[near[:100]]
    h0[near[100:]] = LIMIT - ql[near[100:]]
    pool, ref, qer = pack_pairs(qs, ts, h0)
    w = 100
    oo, go = _opts()
    want, cells = _oracle_per_task(pool, ref, qer, w, oo)
    pcls = bsw_class(pool["len2"], pool["h0"], 1)
    assert set(np.unique(pcls)) == set(range(6))
    rng = np.random.default_rng(17)
    # a class launch of the packed kernel starts 4 * min(ceil(n / 4), 8 CUs) waves and a wave's first ticket is 16 tasks: with
    # n >= 32 CUs, more than 512 CUs tasks in a class make some wave of it take a second ticket and refill its slots mid-wave
    per = 512 * cus + 64 * cus
    sel = np.concatenate([rng.choice(np.flatnonzero(pcls == c), size=per if c < 5 else 20_000) for c in range(6)])
    rng.shuffle(sel)
    n = len(sel)
    counts = np.bincount(pcls[sel], minlength=6)
    bound = 16 * 4 * min(-(-n // 4), 8 * cus)
    print(f"refill: {cus} CUs, {n} tasks from a pool of {len(pool)}, per class {counts.tolist()}, first tickets cover {bound}")
    assert (counts[:5] > bound).all(), (counts, bound)
    big = pool[sel]
    big["id"] = np.arange(n)
    return dict(big=big, ref=ref, qer=qer, want=want[sel], cells=int(cells[sel].sum()), w=w, go=go, n=n)


def test_refill_under_load(ix, knob, refill_set):
    s = refill_set
    big, n = s["big"], s["n"]
    b = capi.Batch(ix, 8, 1200)
    perm = np.random.default_rng(3).permutation(n)
    for order, what in ((np.arange(n), "tiled"), (perm, "permuted")):          # the second run reuses the batch's buffers
        p = np.ascontiguousarray(big[order])
        b.bsw_upload(p, s["ref"], s["qer"])
        b.bsw_run(s["w"], s["go"])
        got = b.bsw_fetch()
        assert_pairs_equal(got, s["want"][order], f"refill {what}, BWAMS_BSW_PK={knob}")
        assert b.stats().bsw_cells == s["cells"], what
        for f in IN_FIELDS:
            assert np.array_equal(got[f], p[f]), (what, f)
    b.close()


# ---- the classes' query-length edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [100, 5])
def test_class_boundaries(ix, knob, w):
    pairs, ref, qer = bsw_class_edge_tasks(w)
    assert set(np.unique(bsw_class(pairs["len2"], pairs["h0"], 1))) == set(range(6))
    _check(ix, pairs, ref, qer, w, what=f"class edges w={w}")


# ---- the score bounds of the packed classes ------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [1, 5])
def test_score_limits(ix, knob, a):
    """The bound h0 + qlen * a at 2^14 - 1 (packed), 2^14 and 2^14 + 1 (one task per wave) at every class edge, reached by
    identical pairs; h0 far beyond it, 0 and negative (util.bsw_score_limit_tasks)."""
    pairs, ref, qer = bsw_score_limit_tasks(a)
    cls = bsw_class(pairs["len2"], pairs["h0"], a)
    top = pairs["h0"].astype(np.int64) + pairs["len2"] * a
    assert ((top == LIMIT - 1) & (cls < 5)).sum() == 10 * 8 and ((top == LIMIT) & (cls == 5)).sum() == 11 * 8
    assert (pairs["h0"] < 0).sum() > 0 and cls[pairs["h0"] < 0].min() == 5
    want = _check(ix, pairs, ref, qer, 100, _opts(a=a), f"score limits a={a}")
    assert (want["score"][(top == LIMIT - 1) & (cls < 5)] == LIMIT - 1).any()     # the packed classes reach their largest score


# ---- bands every cell of which stays positive ----------------------------------------------------------------------------
@pytest.mark.parametrize("w", BSW_WIDE_W)
def test_wide_bands(ix, knob, w):
    """w = 0 is accepted and gives the oracle's one-column band; 700 is wider than every query here."""
    pairs, ref, qer = bsw_wide_band_tasks()
    _check(ix, pairs, ref, qer, w, what=f"wide band w={w}")
    if w >= 33:                                              # rows wider than one 32-column window
        _, cells = _oracle_per_task(pairs, ref, qer, w, _opts()[0])
        assert (cells > 40 * pairs["len1"]).any()


# ---- N ---------------------------------------------------------------------------------------------------------------
def test_n_runs(ix, knob):
    pairs, ref, qer = bsw_n_run_tasks()
    _check(ix, pairs, ref, qer, 100, what="N runs")


# ---- scoring at the edge of what the packed kernel takes -----------------------------------------------------------------
@pytest.mark.parametrize("a,gaps,n_score", BSW_SCORING_EDGES, ids=lambda v: str(v).replace(" ", ""))
def test_pk_eligibility_edges(ix, knob, a, gaps, n_score):
    pairs, ref, qer = bsw_scoring_edge_tasks(a, seed=sum(gaps) + a)
    _check(ix, pairs, ref, qer, 100, _opts(a=a, gaps=gaps, n_score=n_score), f"scoring {a} {gaps} {n_score}")


# ---- long queries: the one-task-per-wave kernel at 4, 3, 2 and 1 waves per block -----------------------------------------
@pytest.mark.parametrize("qmax", [4543, 4544, 6059, 6060, 9094, 9095, MAX_QLEN])
def test_long_queries(ix, knob, qmax):
    rng = np.random.default_rng(qmax)
    q = rng.integers(0, 4, size=qmax, dtype=np.uint8)
    q[rng.random(qmax) < 0.01] = 4
    qs, ts, hs = [], [], []
    for t, h0 in ((q[:400], 30), (mutate(rng, q[:600], 0.05), 60), (q[:300], 3000), (rng.integers(0, 4, 300, dtype=np.uint8), 5000),
                  (q, 10)):
        qs.append(q); ts.append(t); hs.append(h0)
    sq, st, sh = make_task_pool(200, 1, 400, seed=qmax, tlen_max=400)        # short ones in the same launches
    pairs, ref, qer = pack_pairs(qs + sq, ts + st, np.concatenate([hs, sh]))
    _check(ix, pairs, ref, qer, 100, what=f"qmax={qmax}")


def test_query_past_the_lds_limit_is_refused(ix, knob):
    rng = np.random.default_rng(5)
    q = rng.integers(0, 4, size=MAX_QLEN + 1, dtype=np.uint8)
    pairs, ref, qer = pack_pairs([q, q[:50]], [q[:100], q[:50]], [20, 20])
    b = capi.Batch(ix, 8, 1200)
    with pytest.raises(capi.BwamsError) as e:
        b.bsw(pairs, ref, qer, 100)
    assert e.value.code == ERR_UNSUPPORTED
    with pytest.raises(capi.BwamsError) as e:
        b.bsw_upload(pairs, ref, qer)
    assert e.value.code == ERR_UNSUPPORTED
    # the batch stays usable
    pairs, ref, qer = make_pairs(300, seed=6)
    _check(b, pairs, ref, qer, 100, what="after a refused upload")
    b.close()
