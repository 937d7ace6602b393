"""The pass of bsw_pk_kernel (csrc/bsw_extend.hip) at the smallest shapes at which each of its pieces can go wrong, against the
scalar oracle (loader.bsw_pairs): the column masks and the masked write-back, the first / last column with a non-zero stored cell,
the row maximum with the last column attaining it, the carries from one 32-column window of a row to the next, and N bases at
lane and window boundaries.

The harness is that of tests/test_gpu_bsw.py: Batch.bsw with BWAMS_BSW_PK=1 (the packed kernel) and BWAMS_BSW_PK=0 (the
eight-task kernel); the six outputs bit for bit, the DP cell count, the inputs unchanged.  A lane of the packed kernel owns
eight columns and a task's quad a window of 32 that starts at a multiple of four; queries stay within 191 bases.

Every set is built once, with the oracle's answers, and is checked there (before any GPU is asked) to hold tasks that stop
short of the query's end, tasks that never reach it, tasks that do, tasks whose maximum lies off the diagonal and tasks whose
score never exceeds h0."""
import functools

import numpy as np
import pytest

from bwams import capi
from oracle import loader
from util import assert_pairs_equal, bsw_class, bsw_sw_opt, mutate, pack_pairs, toy

IN_FIELDS = ("idr", "idq", "id", "len1", "len2", "h0", "seqid", "regid")
MASK_W = (1, 2, 3, 5, 8)
WINDOW_QLEN = (33, 64, 65, 96, 97, 144, 191)
EDGES = (0, 1, 3, 4, 7, 8, 9, 15, 16, 17, 23, 24, 31, 32, 33, 35, 36, 39, 40, 63, 64, 65, 95, 96, 97)   # lane, window and class edges


def _rnd(rng, n):
    return rng.integers(0, 4, size=int(n), dtype=np.uint8)


def _sub(rng, s, pos):
    """s with the bases at pos replaced by other bases"""
    s = s.copy()
    pos = np.asarray(pos, np.int64)
    s[pos] = (s[pos] + rng.integers(1, 4, size=len(pos))) & 3
    return s


def _assert_not_degenerate(pairs, want, what):
    assert (pairs["len2"] <= 191).all() and (bsw_class(pairs["len2"], pairs["h0"], 1) < 5).all(), what
    kinds = {"qle < len2": want["qle"] < pairs["len2"], "gscore == -1": want["gscore"] == -1, "gscore >= 0": want["gscore"] >= 0,
             "max_off > 0": want["max_off"] > 0, "score never above h0": want["score"] == pairs["h0"]}
    for k, m in kinds.items():
        assert m.any(), f"{what}: no task with {k}"


# ---- the sets -------------------------------------------------------------------------------------------------------
def _mask_tasks(w, noisy):
    """Query lengths 1 .. 72, every value, four tasks each; targets of qlen + w + 3 bases.  With the band w the first and the last
    live column of the rows take every residue mod 8 at every lane of the quad, the last one on lane and window boundaries.
    noisy: h0 in 1 .. 8 and frequent mismatches, so that both ends of the band move inwards as cells fall to zero."""
    rng = np.random.default_rng(1000 * w + noisy)
    qs, ts, hs = [], [], []
    for ql in range(1, 73):
        for k in range(4):
            q = _rnd(rng, ql)
            tl = ql + w + 3
            if not noisy:
                t = np.concatenate([q, _rnd(rng, w + 3)])
                h0 = int(rng.integers(20, 60))
            else:
                t = np.concatenate([mutate(rng, q, (0.1, 0.2, 0.3, 0.5)[k]), _rnd(rng, tl)])[:tl]
                h0 = int(rng.integers(1, 9))
            qs.append(q); ts.append(t); hs.append(h0)
    return pack_pairs(qs, ts, hs)


def _nonzero_tasks():
    """Leading and trailing zero runs in the stored row: the first and the last 1 .. 12 bases of the query mismatch the target.
    Low h0 gives rows with a single live cell and rows of zeros; h0 above o_del + e_del keeps column 0 alive, so that a row starts
    at column 0 with h1 != 0; with h0 >= 200 and an exact middle the rows span two and three windows, the first non-zero column in
    the first window and the last in the last."""
    rng = np.random.default_rng(5)
    qs, ts, hs = [], [], []
    for ql in (13, 24, 25, 31, 32, 33, 40, 64, 65, 72, 96, 97, 120):
        for k1 in (0, 1, 2, 3, 5, 8, 12):
            for k2 in (0, 1, 4, 7, 12):
                if k1 + k2 >= ql:
                    continue
                q = _rnd(rng, ql)
                t = _sub(rng, q, np.concatenate([np.arange(k1), np.arange(ql - k2, ql)]))
                t = np.concatenate([t, _rnd(rng, int(rng.integers(0, 30)))])
                for h0 in (1, 2, 9, 30, 200 + 10 * k1):
                    qs.append(q); ts.append(t); hs.append(h0)
    for ql in (40, 70, 100):                                     # indels behind a mismatching head: the maximum leaves the diagonal
        for rate in (0.05, 0.15):
            for rep in range(6):
                q = _rnd(rng, ql)
                t = np.concatenate([_sub(rng, q[:6], np.arange(3)), mutate(rng, q[6:], rate), _rnd(rng, 20)])
                qs.append(q); ts.append(t); hs.append(int(rng.integers(3, 40)))
    return pack_pairs(qs, ts, hs)


def _tie_tasks():
    """Homopolymers and period-2 queries against the same target: many columns tie for the row maximum and the last one wins.
    With h0 >= 200 the band is wide: the maximum lies in the second window, ties between two windows, ties across the lanes of
    a quad.  Targets shorter and longer than the query, and a foreign base in the target that splits the run."""
    rng = np.random.default_rng(6)
    qs, ts, hs = [], [], []
    for ql in (3, 4, 5, 8, 9, 16, 31, 32, 33, 36, 40, 63, 64, 65, 70, 100, 150):
        for unit in ((0,), (2, 3), (1, 1, 2)):
            q = np.resize(np.array(unit, np.uint8), ql)
            for tl in (max(1, ql // 2), ql, ql + 7, ql + 40):
                t = np.resize(np.array(unit, np.uint8), tl)
                for h0 in (1, 7, 40, 250):
                    qs.append(q); ts.append(t); hs.append(h0)
                t2 = t.copy()
                t2[tl // 2] = (t2[tl // 2] + 1) & 3
                qs.append(q); ts.append(t2); hs.append(int(rng.integers(5, 300)))
                qs.append(q); ts.append(np.concatenate([t[:tl // 3], t[tl // 3 + 2:]])); hs.append(int(rng.integers(5, 300)))
    return pack_pairs(qs, ts, hs)


def _window_tasks():
    """Rows of several windows: h0 >= 200 and w = 100 keep the band wide at every query length at which the number of windows or
    the last window's fill changes.  The carries c_max (the prefix maximum of F) and c_h (the last column's H) cross the window
    boundary: an insertion opens in one window and is extended into the next; deletions and mismatches at the boundaries."""
    rng = np.random.default_rng(7)
    qs, ts, hs = [], [], []
    for ql in WINDOW_QLEN:
        base_t = _rnd(rng, ql + 30)
        for p in (0, 3, 28, 30, 31, 32, 33, 60, 62, 63, 64, 65, 94, 95, 96, 97, 127, 128, 143, 160):
            if p >= ql - 1:
                continue
            for glen in (1, 2, 5, 9):
                q = np.concatenate([base_t[:p], _rnd(rng, glen), base_t[p:]])[:ql]          # an insertion in the query at column p
                qs.append(q); ts.append(base_t); hs.append(int(rng.integers(200, 400)))
            q = base_t[:ql].copy()
            qs.append(q); ts.append(np.concatenate([base_t[:p], _rnd(rng, 4), base_t[p:]])); hs.append(int(rng.integers(200, 400)))   # a deletion
            qs.append(_sub(rng, q, [p, p + 1])); ts.append(base_t); hs.append(int(rng.integers(200, 400)))
        q = base_t[:ql].copy()
        for tl in (ql // 3, ql - 1, ql, ql + 30):                                          # exact, the target shorter and longer
            qs.append(q); ts.append(base_t[:tl]); hs.append(200)
        qs.append(q); ts.append(_rnd(rng, ql)); hs.append(210)                                # unrelated: the band dies from a wide start
        qs.append(q); ts.append(_rnd(rng, ql)); hs.append(2)
    return pack_pairs(qs, ts, hs)


def _n_tasks():
    """N in the query, in the target and in both, single bases and runs, at lane and window boundaries; targets that end just
    behind the N, so that the query's end is never reached."""
    rng = np.random.default_rng(8)
    qs, ts, hs = [], [], []
    for ql in (8, 9, 32, 33, 40, 64, 65, 100, 120):               # 120: beyond the band of row 0, whose end the query's end then is not
        for e in EDGES:
            if e >= ql:
                continue
            for run in (1, 2, 9):
                for where in (0, 1, 2):
                    q = _rnd(rng, ql)
                    t = np.concatenate([mutate(rng, q, (0.0, 0.05)[run % 2]), _rnd(rng, 12)])
                    if where != 1:
                        q[e:e + run] = 4
                    if where != 0:
                        t[e:e + run] = 4
                    if run == 2 and where == 2 and e + 3 < ql:            # the target ends inside the query, just behind the N
                        t = t[:e + 3]
                    qs.append(q); ts.append(t); hs.append(int(rng.choice([2, 15, 60, 250])) if len(t) > ql else 2)
    return pack_pairs(qs, ts, hs)


@functools.lru_cache(maxsize=None)
def task_set(name):
    """(list of (pairs, ref, qer, w, want, cells)) of a named set; the oracle runs once per set"""
    if name == "masks":
        parts = [(_mask_tasks(w, noisy), w) for w in MASK_W for noisy in (0, 1)]
    else:
        parts = [({"nonzero": _nonzero_tasks, "ties": _tie_tasks, "windows": _window_tasks, "n": _n_tasks}[name](), 100)]
        if name == "ties":
            parts.append((parts[0][0], 5))
    oo = bsw_sw_opt(loader)
    out = []
    for (pairs, ref, qer), w in parts:
        want, cells = loader.bsw_pairs(pairs, ref, qer, w, oo)
        out.append((pairs, ref, qer, w, want, cells))
    allp = np.concatenate([o[0] for o in out]); allw = np.concatenate([o[4] for o in out])
    _assert_not_degenerate(allp, allw, name)
    return out


SETS = ("masks", "nonzero", "ties", "windows", "n")


@pytest.mark.parametrize("name", SETS)
def test_sets_are_not_degenerate(name):
    """runs without a GPU: the oracle's answers on every set (task_set asserts), the sizes the suite's time allows"""
    parts = task_set(name)
    for pairs, _, _, _, want, cells in parts:
        assert 200 <= len(pairs) <= 2600 and len(want) == len(pairs) and cells > 0
    if name == "windows":                                          # rows wider than one and than two windows do occur
        pairs, ref, qer, w, _, _ = parts[0]
        wide = pairs[(pairs["len2"] >= 97) & (pairs["h0"] >= 200)][:1]
        assert loader.bsw_pairs(wide, ref, qer, w, bsw_sw_opt(loader))[1] > 64 * 20


# ---- on the GPU ----------------------------------------------------------------------------------------------------------
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


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_pass(ix, knob, name):
    go = bsw_sw_opt(capi)
    b = capi.Batch(ix, 8, 1200)
    try:
        for pairs, ref, qer, w, want, cells in task_set(name):
            what = f"{name} w={w} BWAMS_BSW_PK={knob}"
            got = b.bsw(pairs, ref, qer, w, go)
            assert_pairs_equal(got, want, what)
            assert b.stats().bsw_cells == cells, what
            for f in IN_FIELDS:
                assert np.array_equal(got[f], pairs[f]), (what, f)
    finally:
        b.close()
