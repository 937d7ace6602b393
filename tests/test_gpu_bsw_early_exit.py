"""The early exit of bsw_pk_kernel (csrc/bsw_extend.hip; DESIGN.md, "BSW kernel: the early exit") where the rule can go wrong: a later
row that ties gscore, a band that never reaches the last column, live state right of the window when the w clip slides, the
first-column source, a second maximum behind a long deletion, rows of several windows, a last useful row at tlen - 1, N, and slots
refilled after a rule exit.

The harness is that of tests/test_gpu_bsw_pass.py: Batch.bsw with BWAMS_BSW_PK=1 and =0, here with BWAMS_BSW_EARLY=1.  The packed
kernel must give the oracle's six outputs and compute exactly the cells of the scalar loop with the rule (tests/bsw_early_ref.c);
the 32-bit kernels (BWAMS_BSW_PK=0) do not have the rule: the oracle's outputs and the oracle's cells.  Every set is checked on the
oracle and the restatement, before any GPU is asked, to hold tasks the rule shortens and tasks it must not shorten."""
import functools

import numpy as np
import pytest

from bsw_early import EarlyRef
from bwams import capi
from oracle import loader
from util import OUT_FIELDS, assert_pairs_equal, bsw_class, bsw_sw_opt, make_task_pool, mutate, pack_pairs, toy

IN_FIELDS = ("idr", "idq", "id", "len1", "len2", "h0", "seqid", "regid")
SETS = ("a_tie", "b_never_ends", "c_clip", "d_first_column", "e_second_maximum", "f_wide", "g_last_row", "h_n", "i_refill")


def _rnd(rng, n):
    return rng.integers(0, 4, size=int(n), dtype=np.uint8)


def _sub(rng, s, pos):
    s = s.copy()
    pos = np.asarray(pos, np.int64)
    s[pos] = (s[pos] + rng.integers(1, 4, size=len(pos))) & 3
    return s


def _plain(rng, qs, ts, hs, n, ql_lo, ql_hi, h_lo=19, h_hi=120):
    """exact and lightly mutated copies with a long random tail: the tasks the rule is there for"""
    for _ in range(n):
        q = _rnd(rng, rng.integers(ql_lo, ql_hi + 1))
        t = np.concatenate([mutate(rng, q, float(rng.choice([0.0, 0.0, 0.02, 0.06]))), _rnd(rng, len(q) + 10)])
        qs.append(q); ts.append(t); hs.append(int(rng.integers(h_lo, h_hi)))


def _a_tie():
    """The query ends in a run of period 4; the target holds, in front of that run, k bases that cost the diagonal path m mismatches
    and a deletion 6 + k = 5 m: the row k below the query's last ties gscore, and gtle must move to it.  One mismatch more or less and
    there is no tie."""
    rng = np.random.default_rng(11)
    qs, ts, hs = [], [], []
    for rep in range(700):
        k, m = (4, 2) if rep % 3 else (9, 3)
        unit = rng.permutation(4).astype(np.uint8)
        run = np.resize(unit, int(rng.integers(k + 2, 40)))
        if k == 9:
            unit = np.concatenate([unit, unit, unit[:1]])[:9]
            run = np.resize(unit, int(rng.integers(k + 2, 40)))
        x = _rnd(rng, rng.integers(1, 100))
        d = _sub(rng, run[:k], rng.choice(k, size=m + int(rng.integers(-1, 2)) * (rep % 5 == 0), replace=False))
        q = np.concatenate([x, run])
        t = np.concatenate([x, d, run, _rnd(rng, rng.integers(0, 30))])
        qs.append(q); ts.append(t); hs.append(int(rng.integers(15, 150)))
    _plain(rng, qs, ts, hs, 300, 10, 150)
    return pack_pairs(qs, ts, hs), 100


def _b_never_ends():
    """gscore stays -1 although the score is high: the target ends before the query does, or the query's tail matches nothing"""
    rng = np.random.default_rng(12)
    qs, ts, hs = [], [], []
    for _ in range(500):
        q = _rnd(rng, rng.integers(90, 192))
        cut = int(rng.integers(40, len(q) - 30))
        if rng.random() < 0.5:
            t = mutate(rng, q[:cut], 0.02)                                          # the target stops short
        else:
            t = np.concatenate([q[:cut], _rnd(rng, len(q))])                       # unrelated behind the cut
        qs.append(q); ts.append(t); hs.append(int(rng.integers(19, 40)))          # row -1 dies long before the last column
    _plain(rng, qs, ts, hs, 300, 30, 191)
    return pack_pairs(qs, ts, hs), 100


def _c_clip():
    """w of 5 .. 20 and h0 >= 100 with qlen > w + 1: row -1 is alive far to the right of the band, the clip slides over it"""
    rng = np.random.default_rng(13)
    out = []
    for w in (5, 8, 13, 20):
        qs, ts, hs = [], [], []
        for _ in range(250):
            q = _rnd(rng, rng.integers(w + 2, 192))
            kind = rng.integers(0, 4)
            t = mutate(rng, q, (0.0, 0.03, 0.1, 0.0)[kind])
            if kind == 3:                                                          # a deletion as wide as the band allows
                p = int(rng.integers(1, len(q)))
                t = np.concatenate([q[:p], _rnd(rng, rng.integers(1, w + 2)), q[p:]])
            t = np.concatenate([t, _rnd(rng, rng.integers(0, len(q) + 20))])
            qs.append(q); ts.append(t); hs.append(int(rng.integers(100, 400)))
        out.append((pack_pairs(qs, ts, hs), w))
    return out


def _d_first_column():
    """queries of 1 .. 8 bases with h0 far above: column 0's value h0 - o_del - e_del (i + 1) feeds every row"""
    rng = np.random.default_rng(14)
    qs, ts, hs = [], [], []
    for ql in range(1, 9):
        for _ in range(60):
            q = _rnd(rng, ql)
            tl = int(rng.integers(1, 120))
            t = _rnd(rng, tl)
            if rng.random() < 0.7:
                at = int(rng.integers(0, max(1, tl - ql)))
                t[at:at + ql] = q[:len(t[at:at + ql])]
            qs.append(q); ts.append(t); hs.append(int(rng.choice([20, 60, 100, 300, 1000, 4000])))
    _plain(rng, qs, ts, hs, 200, 1, 8, 8, 40)
    return pack_pairs(qs, ts, hs), 100


def _e_second_maximum():
    """the query's second half lies 10 .. 45 target bases further down: after the deletion the score climbs above the first maximum"""
    rng = np.random.default_rng(15)
    qs, ts, hs = [], [], []
    for _ in range(500):
        a, b = _rnd(rng, rng.integers(10, 70)), _rnd(rng, rng.integers(55, 120))
        gap = int(rng.integers(10, 46))
        t = np.concatenate([a, _rnd(rng, gap), mutate(rng, b, float(rng.choice([0.0, 0.02]))), _rnd(rng, rng.integers(0, 60))])
        qs.append(np.concatenate([a, b])); ts.append(t); hs.append(int(rng.integers(19, 120)))
    _plain(rng, qs, ts, hs, 200, 60, 190)
    return pack_pairs(qs, ts, hs), 100


def _f_wide():
    """h0 >= 200 and w = 100: bands of two to six windows, with indels that cross the window boundaries"""
    rng = np.random.default_rng(16)
    qs, ts, hs = [], [], []
    for _ in range(500):
        q = _rnd(rng, rng.integers(40, 192))
        t = np.concatenate([mutate(rng, q, float(rng.choice([0.0, 0.03, 0.08]))), _rnd(rng, rng.integers(0, 200))])
        if rng.random() < 0.25:
            t = t[:int(rng.integers(5, len(q)))]                                    # ends inside the query: nothing to cut short
        qs.append(q); ts.append(t); hs.append(int(rng.integers(200, 600)))
    return pack_pairs(qs, ts, hs), 100


def _g_last_row():
    """the target ends where the query does, or a row or two around it: the last useful row is tlen - 1"""
    rng = np.random.default_rng(17)
    qs, ts, hs = [], [], []
    for _ in range(600):
        q = _rnd(rng, rng.integers(2, 192))
        t = mutate(rng, q, float(rng.choice([0.0, 0.0, 0.03])))
        d = int(rng.integers(-2, 4))
        t = t[:len(t) + d] if d < 0 else np.concatenate([t, _rnd(rng, d)])
        if len(t) == 0:
            t = q[:1]
        qs.append(q); ts.append(t); hs.append(int(rng.integers(10, 200)))
    _plain(rng, qs, ts, hs, 200, 20, 190)
    return pack_pairs(qs, ts, hs), 100


def _h_n():
    """N in the query, in the target and in both, single bases and runs"""
    rng = np.random.default_rng(18)
    qs, ts, hs = [], [], []
    for _ in range(800):
        q = _rnd(rng, rng.integers(8, 192))
        t = np.concatenate([mutate(rng, q, float(rng.choice([0.0, 0.03]))), _rnd(rng, len(q))])
        for s in ((q,), (t,), (q, t))[int(rng.integers(0, 3))]:
            at, run = int(rng.integers(0, len(q))), int(rng.choice([1, 1, 2, 9]))
            s[at:at + run] = 4
        if rng.random() < 0.25:
            t = t[:int(rng.integers(3, len(q)))]                                    # ends inside the query: nothing to cut short
        qs.append(q); ts.append(t); hs.append(int(rng.integers(15, 250)))
    return pack_pairs(qs, ts, hs), 100


N_REFILL = 150000            # a launch has at most 8192 waves of sixteen slots: 131 072 tasks fill every slot once


def _i_refill():
    """more tasks than sixteen times the waves of a launch, lengths of one class mixed: slots are refilled after rule exits"""
    q, t, h = make_task_pool(3000, 32, 63, seed=19, tlen_max=260)
    rng = np.random.default_rng(19)
    pick = rng.integers(0, len(q), size=N_REFILL)
    return pack_pairs([q[k] for k in pick], [t[k] for k in pick], [h[k] for k in pick]), 100


@functools.lru_cache(maxsize=None)
def _ref_lib():
    import tempfile
    return EarlyRef(tempfile.mkdtemp(prefix="bsw_early_"))


@functools.lru_cache(maxsize=None)
def task_set(name):
    """list of (pairs, ref, qer, w, the oracle's pairs, the oracle's cells, the cells with the rule); oracle and restatement run once per set"""
    parts = globals()["_" + name]()
    parts = parts if isinstance(parts, list) else [parts]
    oo = bsw_sw_opt(loader)
    out, n_short, n_same, n_tie = [], 0, 0, 0
    for (pairs, ref, qer), w in parts:
        assert (pairs["len2"] <= 191).all() and (bsw_class(pairs["len2"], pairs["h0"], 1) < 5).all(), name
        want, cells = loader.bsw_pairs(pairs, ref, qer, w, oo)
        off, c0, _, _ = _ref_lib().run(pairs, ref, qer, w, oo, 0)
        got, c1, _, _ = _ref_lib().run(pairs, ref, qer, w, oo, 1)
        assert int(c0.sum()) == cells and (c1 <= c0).all(), name
        for f in OUT_FIELDS:
            assert np.array_equal(got[f], want[f]) and np.array_equal(off[f], want[f]), (name, f)
        n_short += int((c1 < c0).sum()); n_same += int((c1 == c0).sum())
        if name == "a_tie":                                        # the wrong rule, P <= gscore, stops before the row that ties gscore
            bad = _ref_lib().run(pairs, ref, qer, w, oo, 3)[0]
            n_tie += int((bad["gtle"] != want["gtle"]).sum())
        out.append((pairs, ref, qer, w, want, cells, int(c1.sum())))
    print(f"{name}: {n_short} tasks shortened, {n_same} not" + (f", {n_tie} where a later row ties gscore" if name == "a_tie" else ""))
    assert n_short >= 20 and n_same >= 20, (name, n_short, n_same)
    allp = np.concatenate([o[0] for o in out]); allw = np.concatenate([o[4] for o in out])
    if name == "a_tie":
        assert n_tie >= 20, n_tie
    if name == "b_never_ends":
        assert ((allw["gscore"] == -1) & (allw["score"] >= allp["h0"] + 20)).sum() >= 100
    if name == "c_clip":
        assert all(((o[0]["h0"] >= 100) & (o[0]["len2"] > o[3] + 1)).all() for o in out)
    if name == "d_first_column":
        assert ((allp["len2"] <= 8) & (allp["h0"] >= 10 * allp["len2"])).sum() >= 300
    if name == "e_second_maximum":
        assert ((allw["max_off"] >= 10) & (allw["tle"] > allw["qle"] + 9)).sum() >= 100
    if name == "g_last_row":
        assert (allw["gtle"] == allp["len1"]).sum() >= 100 and (allw["tle"] == allp["len1"]).sum() >= 100
    if name == "i_refill":
        assert len(allp) > 16 * 8192
    return out


@pytest.mark.parametrize("name", SETS)
def test_sets_are_not_degenerate(name):
    """runs without a GPU: what task_set asserts of every set, and the sizes the suite's time allows"""
    for pairs, _, _, _, want, cells, early in task_set(name):
        assert len(want) == len(pairs) and 0 < early <= cells
        assert name == "i_refill" or 200 <= len(pairs) <= 3000
    if name == "f_wide":
        assert any(int(loader.bsw_pairs(p[k:k + 1], r, q, w, bsw_sw_opt(loader))[1]) > 64 * 20 for p, r, q, w, *_ in task_set(name) for k in range(20))


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
    monkeypatch.setenv("BWAMS_BSW_EARLY", "1")
    capi.debug_reload()                                    # the switches are read once: say that it changed
    yield request.param
    monkeypatch.undo()
    capi.debug_reload()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_early_exit(ix, knob, name):
    go = bsw_sw_opt(capi)
    b = capi.Batch(ix, 8, 1200)
    try:
        for pairs, ref, qer, w, want, cells, early in task_set(name):
            what = f"{name} w={w} BWAMS_BSW_PK={knob} BWAMS_BSW_EARLY=1"
            got = b.bsw(pairs, ref, qer, w, go)
            assert_pairs_equal(got, want, what)                    # in task order
            n_cells = b.stats().bsw_cells
            print(what, "cells", n_cells, "of the oracle's", cells)
            assert n_cells == (early if knob == "1" else cells) and n_cells <= cells, what
            for f in IN_FIELDS:
                assert np.array_equal(got[f], pairs[f]), (what, f)
    finally:
        b.close()


@pytest.mark.gpu
def test_extend_run_is_the_same_with_and_without(monkeypatch):
    """bwams_extend_run on the small genome of tests/test_gpu_ext_rounds.py with BWAMS_BSW_EARLY unset (the rule on), 0 and 1: the
    fetched regions are byte-equal, and the rule computes fewer cells"""
    from bwams import fmindex, simulate
    from test_gpu_ext_rounds import _batch, _indel_reads, _oracle, _tier_genome
    capi.lib()
    g = _tier_genome()
    idx = fmindex.build_fmindex(g)
    ix = capi.Index.from_host(idx, 0)
    c = np.zeros(1, capi.CONTIG_DTYPE)
    c["len"] = len(g)
    ix.set_contigs(c)
    reads = list(simulate.make_reads(g, 1500, seed=3)[0]) + _indel_reads(g)
    w = _oracle(idx, g, reads, max_occ=2000)
    runs = {}
    try:
        for setting in (None, "0", "1"):
            monkeypatch.delenv("BWAMS_BSW_EARLY", raising=False)
            if setting is not None:
                monkeypatch.setenv("BWAMS_BSW_EARLY", setting)
            capi.debug_reload()
            b = _batch(ix, w)
            b.seed_upload(w["enc"], w["cum"])
            b.seed_run(w["sg"], with_sa=True)
            b.chain_run(w["gopt"])
            n = b.extend_run(w["gopt"])
            regs, reg_off, aln = b.extend_fetch()
            runs[setting] = (n, regs.tobytes(), reg_off.tobytes(), aln.tobytes(), b.stats().bsw_cells)
            b.close()
    finally:
        monkeypatch.undo()
        capi.debug_reload()
        ix.close()
    assert runs[None][0] == len(w["wregs"]) > 0
    for setting in ("0", "1"):
        assert runs[setting][:4] == runs[None][:4], setting
    print("bsw_cells: unset", runs[None][4], "BWAMS_BSW_EARLY=0", runs["0"][4], "=1", runs["1"][4])
    assert runs[None][4] == runs["1"][4] < runs["0"][4]
